"""Image element (reference: vkit/element/image.py).

uint8 HxW[xC] (or float32 for the ``*_GCN`` modes) plus an ``ImageMode`` tag.  Mode conversion on the hot
path is RGB <-> HSV (``cv.COLOR_RGB2HSV_FULL`` / ``cv.COLOR_HSV2RGB_FULL``, reference image.py:188-202,771-814)
and runs in the ``k_hsv`` HIP kernel; other conversions are outside the accelerated path and raise.
"""
from enum import Enum, unique
from typing import Optional, Tuple, Union

import attrs
import numpy as np

from ._writable import LazyMat, WritableContext
from .opt import generate_shape_and_resized_shape
from .type import ElementSetOperationMode, Shapable


@unique
class ImageMode(Enum):
    RGB = 'rgb'
    RGB_GCN = 'rgb_gcn'
    RGBA = 'rgba'
    HSV = 'hsv'
    HSV_GCN = 'hsv_gcn'
    HSL = 'hsl'
    HSL_GCN = 'hsl_gcn'
    GRAYSCALE = 'grayscale'
    GRAYSCALE_GCN = 'grayscale_gcn'
    NONE = 'none'

    def to_ndim(self):
        if self in (ImageMode.GRAYSCALE, ImageMode.GRAYSCALE_GCN):
            return 2
        if self is ImageMode.NONE:
            raise NotImplementedError()
        return 3

    def to_dtype(self):
        if self is ImageMode.NONE:
            raise NotImplementedError()
        return np.float32 if self.in_gcn_mode() else np.uint8

    def to_num_channels(self):
        if self is ImageMode.RGBA:
            return 4
        if self in (ImageMode.GRAYSCALE, ImageMode.GRAYSCALE_GCN):
            return None
        if self is ImageMode.NONE:
            raise NotImplementedError()
        return 3

    def supports_gcn_mode(self):
        # the reference's test is inverted (vkit/element/image.py:69-72: ``self not in _IMAGE_MODE_NON_GCN_TO_GCN``): a mode WITH a
        # GCN twin answers False -- to_gcn_mode() and with it to_gcn_image() raise RuntimeError for RGB / GRAYSCALE / HSV / HSL, and
        # KeyError for the rest.  Kept: a drop-in behaves like what it replaces (tests/golden/gcn.npz records the reference's answers)
        return self not in _TO_GCN

    def to_gcn_mode(self):
        if not self.supports_gcn_mode():
            raise RuntimeError(f'image_mode={self} not supported.')
        return _TO_GCN[self]

    def in_gcn_mode(self):
        return self in _FROM_GCN

    def to_non_gcn_mode(self):
        if not self.in_gcn_mode():
            raise RuntimeError(f'image_mode={self} not in gcn mode.')
        return _FROM_GCN[self]


_TO_GCN = {
    ImageMode.RGB: ImageMode.RGB_GCN,
    ImageMode.HSV: ImageMode.HSV_GCN,
    ImageMode.HSL: ImageMode.HSL_GCN,
    ImageMode.GRAYSCALE: ImageMode.GRAYSCALE_GCN,
}
_FROM_GCN = {gcn: plain for plain, gcn in _TO_GCN.items()}


@attrs.define
class ImageSetItemConfig:
    value: Union['Image', np.ndarray, Tuple[int, ...], int]
    alpha: Union[np.ndarray, float] = 1.0


@attrs.define(frozen=True, eq=False)
class Image(LazyMat, Shapable):
    _mat: np.ndarray = attrs.field(alias='mat')
    mode: ImageMode = ImageMode.NONE
    box: Optional['Box'] = None

    def __attrs_post_init__(self):
        if self.mode != ImageMode.NONE:
            assert self.mode.to_dtype() == self._mat.dtype
            assert self.mode.to_ndim() == self._mat.ndim
        else:
            # infer the mode from the array (uint8 only)
            if self._mat.dtype == np.float32:
                raise NotImplementedError('mode is None and mat.dtype == np.float32.')
            if self._mat.dtype != np.uint8:
                raise NotImplementedError(f'Invalid mat.dtype={self._mat.dtype}.')
            if self._mat.ndim == 2:
                mode = ImageMode.GRAYSCALE
            elif self._mat.ndim == 3 and self._mat.shape[2] == 4:
                mode = ImageMode.RGBA
            elif self._mat.ndim == 3 and self._mat.shape[2] == 3:
                mode = ImageMode.RGB
            elif self._mat.ndim == 3:
                raise NotImplementedError(f'Invalid num_channels={self._mat.shape[2]}.')
            else:
                raise NotImplementedError(f'mat.ndim={self._mat.ndim} not supported.')
            object.__setattr__(self, 'mode', mode)
        if isinstance(self._mat, np.ndarray):
            self._mat.flags.writeable = False
        if self.box and self.shape != self.box.shape:
            raise RuntimeError('self.shape != box.shape.')

    # ---- constructors
    @classmethod
    def from_shape(cls, shape: Tuple[int, int], num_channels: int = 3, value: Union[Tuple[int, ...], int] = 255):
        height, width = shape
        if num_channels == 0:
            mat_shape = (height, width)
        else:
            assert num_channels > 0
            if isinstance(value, tuple):
                assert len(value) == num_channels
            mat_shape = (height, width, num_channels)
        return cls(mat=np.full(mat_shape, fill_value=value, dtype=np.uint8))

    @classmethod
    def from_shapable(cls, shapable: Shapable, num_channels: int = 3, value: Union[Tuple[int, ...], int] = 255):
        return cls.from_shape(shapable.shape, num_channels=num_channels, value=value)

    @classmethod
    def from_pil_image(cls, pil_image):
        # an explicit copy: the array of a PIL image is not writable
        return cls(mat=np.array(pil_image, dtype=np.uint8))

    @classmethod
    def from_file(cls, path, disable_exif_orientation: bool = False):
        """The decoded file (reference image.py:325-349): Pillow ``open`` + ``load``, the EXIF orientation applied unless
        disabled, the mode inferred from the decoded array (2-D: GRAYSCALE, 3 channels: RGB, 4: RGBA)."""
        import os
        from PIL import Image as PilImage, ImageOps as PilImageOps
        # PilImage.open cannot handle `~`
        pil_image = PilImage.open(os.path.expanduser(os.fspath(path)))
        pil_image.load()
        if not disable_exif_orientation:
            # tag 0x0112; transposed only when set, which avoids a copy
            if pil_image.getexif().get(0x0112):
                pil_image = PilImageOps.exif_transpose(pil_image)
        return cls.from_pil_image(pil_image)

    def to_pil_image(self):
        from PIL import Image as PilImage
        return PilImage.fromarray(self.mat)

    def to_jpeg_bytes(self, quality: int = 75):
        """The file ``to_pil_image().save(f, format='JPEG', quality=quality)`` writes, encoded on the device (csrc/jpeg_encode.hip):
        a 2-D mat as one component, a 3-channel mat with channel 0 as red."""
        return encode_jpeg_images([self], quality=quality)[0]

    def to_file(self, path, disable_to_rgb_image: bool = False):
        """The image written to ``path`` (reference image.py:351-359): converted to RGB unless disabled, then saved as Pillow saves
        it by the path's extension.  A uint8 image of 1 or 3 channels under an extension Pillow writes as JPEG
        (``JPEG_EXTENSIONS``) is encoded on the device, at Pillow's default quality 75 and to the byte the file Pillow writes;
        every other file is Pillow's ``save`` of the host copy."""
        import os
        image = self
        if not disable_to_rgb_image:
            image = image.to_rgb_image()
        # PilImage.save cannot handle `~`
        path = os.path.expanduser(os.fspath(path))
        if os.path.splitext(path)[1].lower() in JPEG_EXTENSIONS and image.arr.dtype == np.uint8:
            if image.num_channels not in (0, 3):
                raise OSError(f'cannot write mode {image.mode.name} as JPEG')        # as Pillow's JPEG plugin answers
            data = image.to_jpeg_bytes()
            with open(path, 'wb') as f:
                f.write(data)
            return
        image.to_pil_image().save(path)

    # ---- properties
    @property
    def height(self):
        return self._mat.shape[0]

    @property
    def width(self):
        return self._mat.shape[1]

    @property
    def num_channels(self):
        return 0 if self._mat.ndim == 2 else self._mat.shape[2]

    @property
    def writable_context(self):
        return WritableContext(self)

    # ---- operators
    def copy(self):
        return attrs.evolve(self, mat=self.mat.copy())

    def assign_mat(self, mat: np.ndarray):
        with self.writable_context:
            object.__setattr__(self, '_mat', mat)

    # ---- fills of a list of elements (reference image.py:371-665): vkit_amd/element/_sets.py
    @classmethod
    def check_values_and_alphas_uniqueness(cls, values, alphas):
        return check_elements_uniqueness(values) and check_elements_uniqueness(alphas)

    @classmethod
    def unpack_element_value_tuples(cls, element_value_tuples):
        """(element, value) or (element, value, alpha) tuples -> elements, values, alphas (1.0 where none is given)."""
        elements, values, alphas = [], [], []
        for element_value_tuple in element_value_tuples:
            if len(element_value_tuple) == 2:
                element, value = element_value_tuple
                alpha = 1.0
            else:
                element, value, alpha = element_value_tuple
            elements.append(element)
            values.append(value)
            alphas.append(alpha)
        return elements, values, alphas

    def _fill_by_tuples(self, kind, tuples, mode, skip_values_uniqueness_check):
        elements, values, alphas = self.unpack_element_value_tuples(tuples)
        _sets.fill_by(self, kind, elements, values, alphas, mode, skip_values_uniqueness_check=skip_values_uniqueness_check)

    def fill_by_box_value_tuples(self, box_value_tuples, mode: ElementSetOperationMode = ElementSetOperationMode.UNION,
                                 skip_values_uniqueness_check: bool = False):
        self._fill_by_tuples(_sets.BOXES, box_value_tuples, mode, skip_values_uniqueness_check)

    def fill_by_boxes(self, boxes, value, alpha: Union[np.ndarray, float] = 1.0,
                      mode: ElementSetOperationMode = ElementSetOperationMode.UNION):
        self.fill_by_box_value_tuples(((box, value, alpha) for box in boxes), mode=mode, skip_values_uniqueness_check=True)

    def fill_by_polygon_value_tuples(self, polygon_value_tuples, mode: ElementSetOperationMode = ElementSetOperationMode.UNION,
                                     skip_values_uniqueness_check: bool = False):
        self._fill_by_tuples(_sets.POLYGONS, polygon_value_tuples, mode, skip_values_uniqueness_check)

    def fill_by_polygons(self, polygons, value, alpha: Union[np.ndarray, float] = 1.0,
                         mode: ElementSetOperationMode = ElementSetOperationMode.UNION):
        self.fill_by_polygon_value_tuples(((polygon, value, alpha) for polygon in polygons), mode=mode,
                                          skip_values_uniqueness_check=True)

    def fill_by_mask_value_tuples(self, mask_value_tuples, mode: ElementSetOperationMode = ElementSetOperationMode.UNION,
                                  skip_values_uniqueness_check: bool = False):
        self._fill_by_tuples(_sets.MASKS, mask_value_tuples, mode, skip_values_uniqueness_check)

    def fill_by_masks(self, masks, value, alpha: Union[np.ndarray, float] = 1.0,
                      mode: ElementSetOperationMode = ElementSetOperationMode.UNION):
        self.fill_by_mask_value_tuples(((mask, value, alpha) for mask in masks), mode=mode, skip_values_uniqueness_check=True)

    def fill_by_score_map_value_tuples(self, score_map_value_tuples,
                                       mode: ElementSetOperationMode = ElementSetOperationMode.UNION,
                                       skip_values_uniqueness_check: bool = False):
        # the score maps are the selection and the alpha: alphas given with them are ignored, as in the reference
        self._fill_by_tuples(_sets.SCORE_MAPS, score_map_value_tuples, mode, skip_values_uniqueness_check)

    def fill_by_score_maps(self, score_maps, value, mode: ElementSetOperationMode = ElementSetOperationMode.UNION):
        self.fill_by_score_map_value_tuples(((score_map, value) for score_map in score_maps), mode=mode,
                                            skip_values_uniqueness_check=True)

    def __setitem__(self, element, config):
        """image[box | polygon | mask | score_map] = value | ImageSetItemConfig (reference image.py:667-712)."""
        if isinstance(config, ImageSetItemConfig):
            value, alpha = config.value, config.alpha
        else:
            value, alpha = config, 1.0
        if isinstance(value, tuple):
            assert value and isinstance(value[0], int)
        if isinstance(element, ScoreMap):
            element.fill_image(image=self, value=value)
        else:
            element.fill_image(image=self, value=value, alpha=alpha)

    def __getitem__(self, element):
        return element.extract_image(self)

    def to_box_attached(self, box: 'Box'):
        assert self.height == box.height and self.width == box.width
        return attrs.evolve(self, box=box)

    def to_box_detached(self):
        assert self.box
        return attrs.evolve(self, box=None)

    def to_resized_image(self, resized_height: Optional[int] = None, resized_width: Optional[int] = None,
                         cv_resize_interpolation: int = 2):
        """cv.resize(mat, (w, h), interpolation) on the GPU (reference image.py:836-852) for cv.INTER_NEAREST (0),
        cv.INTER_LINEAR (1) and the default cv.INTER_CUBIC (2)."""
        from vkit_amd import _native
        if cv_resize_interpolation not in range(7):
            raise ValueError(f'unknown cv2 interpolation code {cv_resize_interpolation}')
        _, _, resized_height, resized_width = generate_shape_and_resized_shape(
            shapable_or_shape=self, resized_height=resized_height, resized_width=resized_width)
        if self._mat.dtype == np.float32 and self._mat.ndim == 3:
            # a float32 (*_GCN) colour image: cv.resize treats the channels alike, so plane by plane through the float32 kernels
            planes = [_native.host_array(_native.resize(np.ascontiguousarray(self.mat[:, :, c]), (resized_height, resized_width),
                                                        cv_resize_interpolation)) for c in range(self._mat.shape[2])]
            return attrs.evolve(self, mat=np.stack(planes, axis=-1))
        return attrs.evolve(self, mat=_native.resize(self.arr, (resized_height, resized_width), cv_resize_interpolation))

    def to_conducted_resized_image(self, shapable_or_shape, resized_height: Optional[int] = None,
                                   resized_width: Optional[int] = None, cv_resize_interpolation: int = 2):
        assert self.box
        resized_box = self.box.to_conducted_resized_box(shapable_or_shape=shapable_or_shape,
                                                        resized_height=resized_height, resized_width=resized_width)
        resized_image = self.to_box_detached().to_resized_image(
            resized_height=resized_box.height, resized_width=resized_box.width,
            cv_resize_interpolation=cv_resize_interpolation)
        return resized_image.to_box_attached(resized_box)

    def to_shifted_image(self, offset_y: int = 0, offset_x: int = 0):
        assert self.box
        return attrs.evolve(self, box=self.box.to_shifted_box(offset_y=offset_y, offset_x=offset_x))

    def to_cropped_image(self, up=None, down=None, left=None, right=None):
        assert not self.box
        up = up or 0
        down = down or self.height - 1
        left = left or 0
        right = right or self.width - 1
        return attrs.evolve(self, mat=self.mat[up:down + 1, left:right + 1])

    def to_gcn_image(self, lamb: float = 0, eps: float = 1E-8, scale: float = 1.0):
        """Global contrast normalisation to the float32 twin of the mode (reference image.py:733-756, numpy only).  As in the
        reference the call cannot get past ``to_gcn_mode()`` (see ``ImageMode.supports_gcn_mode``); the arithmetic below is the
        reference's and is what a fixed reference would compute."""
        mode = self.mode.to_gcn_mode()
        mat = self.mat.astype(np.float32)
        mean = np.mean(mat)
        mat -= mean
        std = np.sqrt(lamb + np.mean(mat**2))
        mat /= max(eps, std)
        if scale != 1.0:
            mat *= scale
        return Image(mat=mat, mode=mode)

    def to_non_gcn_image(self):
        """float32 ``*_GCN`` image -> its uint8 mode: shift to zero, stretch the range to 255, round, clip (reference
        image.py:758-768; numpy expressions, pinned by tests/golden/gcn.npz)."""
        mode = self.mode.to_non_gcn_mode()
        assert self.mat.dtype == np.float32
        val_min = np.min(self.mat)
        mat = self.mat - val_min
        gap = np.max(mat)
        mat = mat / gap * 255.0
        mat = np.round(mat)
        mat = np.clip(mat, 0, 255).astype(np.uint8)
        return Image(mat=mat, mode=mode)

    def to_target_mode_image(self, target_mode: ImageMode):
        """cv.cvtColor chain of the reference (image.py:771-814) among GRAYSCALE / RGB / RGBA / HSV / HSL: the two shortcuts
        GRAYSCALE <-> RGBA, otherwise source -> RGB -> target, HSL stored as HLS with the last two channels swapped.  The
        conversions run on the GPU.  A float32 ``*_GCN`` source is taken to its uint8 mode first (``to_non_gcn_image``), as in the
        reference; a ``*_GCN`` target is as impossible here as there (the reference's conversion table has none)."""
        if target_mode == self.mode:
            return self
        if self.mode.in_gcn_mode():
            self = self.to_non_gcn_image()
            if self.mode == target_mode:
                return self
        from vkit_amd import _native
        supported = (ImageMode.GRAYSCALE, ImageMode.RGB, ImageMode.RGBA, ImageMode.HSV, ImageMode.HSL)
        if self.mode not in supported or target_mode not in supported:
            raise NotImplementedError(
                f'image mode conversion {self.mode} -> {target_mode} is outside the accelerated path')
        mat = self.arr
        if self.mode == ImageMode.HSL:
            mat = self.mat[:, :, [0, 2, 1]]      # HSL -> HLS
        shortcut = {(ImageMode.GRAYSCALE, ImageMode.RGBA): _native.CVT_GRAY2RGBA,
                    (ImageMode.RGBA, ImageMode.GRAYSCALE): _native.CVT_RGBA2GRAY}.get((self.mode, target_mode))
        if shortcut is not None:
            return Image(mat=_native.cvt_color(mat, shortcut), mode=target_mode)
        if self.mode != ImageMode.RGB:
            code = {ImageMode.GRAYSCALE: _native.CVT_GRAY2RGB, ImageMode.RGBA: _native.CVT_RGBA2RGB,
                    ImageMode.HSV: _native.CVT_HSV2RGB_FULL, ImageMode.HSL: _native.CVT_HLS2RGB_FULL}[self.mode]
            mat = _native.cvt_color(mat, code)
        if target_mode == ImageMode.RGB:
            return Image(mat=mat, mode=ImageMode.RGB)
        code = {ImageMode.GRAYSCALE: _native.CVT_RGB2GRAY, ImageMode.RGBA: _native.CVT_RGB2RGBA,
                ImageMode.HSV: _native.CVT_RGB2HSV_FULL, ImageMode.HSL: _native.CVT_RGB2HLS_FULL}[target_mode]
        mat = _native.cvt_color(mat, code)
        if target_mode == ImageMode.HSL:
            mat = _native.host_array(mat)[:, :, [0, 2, 1]]           # HLS -> HSL
        return Image(mat=mat, mode=target_mode)

    def to_rgb_image(self):
        return self.to_target_mode_image(ImageMode.RGB)

    def to_hsv_image(self):
        return self.to_target_mode_image(ImageMode.HSV)

    def to_grayscale_image(self):
        return self.to_target_mode_image(ImageMode.GRAYSCALE)

    def to_hsl_image(self):
        return self.to_target_mode_image(ImageMode.HSL)

    def to_rgba_image(self):
        return self.to_target_mode_image(ImageMode.RGBA)


# the extensions Pillow maps to its JPEG plugin, lower case
JPEG_EXTENSIONS = ('.jpg', '.jpeg', '.jpe', '.jfif')


def encode_jpeg_images(images, quality: int = 75):
    """``image.to_jpeg_bytes(quality)`` for every image of ``images`` (uint8, 1 or 3 channels, any mix of shapes: the crops of a
    page) in ONE device call -> a list of ``bytes``."""
    from vkit_amd import _native
    images = list(images)
    for image in images:
        if image.arr.dtype != np.uint8 or image.num_channels not in (0, 3):
            raise OSError(f'cannot write mode {image.mode.name} as JPEG')
    return _native.jpeg_encode([image.arr for image in images], quality=quality)


from .box import Box  # noqa: E402
from .score_map import ScoreMap  # noqa: E402
from .uniqueness import check_elements_uniqueness  # noqa: E402
from . import _sets  # noqa: E402
