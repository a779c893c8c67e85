"""The selector image engine (reference: vkit/engine/image/selector.py): one file of the configured folders, a random window of
it when the page fits inside and ``force_resize`` is off, else the file resized (INTER_CUBIC) to the page.

The file list is built with the reference's six globs per folder, in its order (``**/*.jpg``, ``**/*.JPG``, ``**/*.jpeg``,
``**/*.JPEG``, ``**/*.png``, ``**/*.PNG``); the order inside one glob is the file system's, there as here, so two machines
may number the files differently.  ``image_files=[...]`` hands the constructor an explicit list instead (a deterministic
order for tests and for jobs that must replay).  Decoded files live on the device in the same kind of cache the combiner
keeps; the window is a device copy (an integer translation through vkx_warp_affine_u8_dev, exact), the resize is
vkx_resize_u8_dev.  A run never hands out the cached texture itself: the whole file is returned as a copy."""
import pathlib
import os
from os import PathLike
from typing import List, Optional, Sequence

import attrs
import numpy as np
from numpy.random import Generator as RandomGenerator

from vkit_amd import _native
from vkit_amd.element import Image, ImageMode
from vkit_amd.utility import rng_choice
from ..interface import EngineExecutorFactory, NoneTypeEngineInitResource
from .cache import TextureCache
from .combiner import DEFAULT_CACHE_BYTES, load_texture
from .type import ImageEngineRunConfig


@attrs.define
class ImageSelectorEngineInitConfig:
    image_folders: Sequence[str]
    target_image_mode: Optional[ImageMode] = ImageMode.RGB
    force_resize: bool = False


class ImageSelectorEngine:

    @classmethod
    def get_type_name(cls) -> str:
        return 'selector'

    def __init__(self, init_config: ImageSelectorEngineInitConfig, init_resource: Optional[NoneTypeEngineInitResource] = None,
                 image_files: Optional[Sequence[PathLike]] = None, cache_bytes: int = DEFAULT_CACHE_BYTES):
        self.init_config = init_config
        self.init_resource = init_resource
        self.image_files: List[PathLike] = []
        if image_files is not None:
            self.image_files.extend(image_files)
        else:
            for image_folder in self.init_config.image_folders:
                image_fd = pathlib.Path(os.path.expandvars(os.fspath(image_folder)))
                if not image_fd.is_dir():
                    raise NotADirectoryError(str(image_fd))
                for ext in ['jpg', 'jpeg', 'png']:
                    for new_ext in [ext, ext.upper()]:
                        self.image_files.extend(image_fd.glob(f'**/*.{new_ext}'))
        self.cache_bytes = int(cache_bytes)
        self._caches = {}

    def texture(self, ctx, image_file):
        """The decoded file as a DevArray of ``ctx`` (None: the thread's default context), from the context's cache."""
        ctx = ctx or _native.default_ctx()
        cache = self._caches.get(id(ctx))
        if cache is None or cache[0]() is not ctx:
            import weakref
            cache = self._caches[id(ctx)] = (weakref.ref(ctx), TextureCache(self.cache_bytes))
        key = os.fspath(image_file)
        arr = cache[1].get(key)
        if arr is None:
            arr = cache[1].put(key, load_texture(ctx, image_file, self.init_config.target_image_mode))
        return arr

    def run(self, run_config: ImageEngineRunConfig, rng: Optional[RandomGenerator] = None) -> Image:
        assert rng is not None
        keep = _native.resident_mode()

        image_file = rng_choice(rng, self.image_files)
        arr = self.texture(_native.default_ctx(), image_file)
        # the mode is inferred from the array, as Image.from_file does; a converted image carries its target mode
        image = Image(mat=arr, mode=self.init_config.target_image_mode or ImageMode.NONE)

        if run_config.disable_resizing:
            assert run_config.height == 0 and run_config.width == 0
            # a copy: the caller may write the image it gets, the cached texture serves every later run
            return attrs.evolve(image, mat=_native.device_copy(arr) if keep else np.array(arr.host()))

        height = run_config.height
        width = run_config.width
        if not self.init_config.force_resize and height <= image.height and width <= image.width:
            # Select a part of image.
            up = int(rng.integers(0, image.height - height + 1))
            left = int(rng.integers(0, image.width - width + 1))
            if (height, width) != image.shape:
                arr = _native.warp_affine(arr, [[1, 0, -left], [0, 1, -up]], (width, height))
            else:
                arr = _native.device_copy(arr)      # the whole file: still a copy, never the cache entry itself
            image = attrs.evolve(image, mat=arr)
        else:
            # Resize image.
            image = image.to_resized_image(resized_height=height, resized_width=width)
        # (outside resident mode the device result is private to this run, and so is its host copy)
        return image if keep else attrs.evolve(image, mat=_native.host_array(image.arr))


image_selector_engine_executor_factory = EngineExecutorFactory(ImageSelectorEngine, ImageSelectorEngineInitConfig,
                                                               ImageEngineRunConfig)
