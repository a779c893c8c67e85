"""CropperState / Cropper (reference: vkit/mechanism/cropper.py).

The geometry is the reference's, statement for statement, and so are its ``rng.integers`` calls: the windows a step draws
depend on nothing else.  The pixels are a device kernel (``vkx_crop_planes_dev``, csrc/crop.hip): a device-resident element
gives a device-resident crop, a host element is uploaded, cropped by the same kernel and handed back on the host.
"""
from typing import Tuple

import attrs
from numpy.random import Generator as RandomGenerator

from vkit_amd import _native
from vkit_amd.element import Box, Image, Mask, Point, ScoreMap


@attrs.define
class CropperState:
    height: int
    width: int
    pad_value: int
    crop_size: int
    original_box: Box
    target_box: Box
    target_core_box: Box
    original_core_box: Box

    @classmethod
    def sample_cropping_positions_along_axis(cls, core_size: int, pad_size: int, crop_size: int, length: int,
                                             rng: RandomGenerator):
        if core_size <= length:
            core_begin = rng.integers(0, length - core_size + 1)
            begin = core_begin - pad_size
            target_offset = 0
            if begin < 0:
                target_offset = abs(begin)
                begin = 0
        else:
            begin = 0
            target_offset = pad_size
            target_offset += rng.integers(0, core_size - length + 1)

        end = min(length - 1, begin + (crop_size - target_offset) - 1)
        return target_offset, begin, end

    @classmethod
    def sample_cropping_positions(cls, height: int, width: int, core_size: int, pad_size: int, crop_size: int,
                                  rng: RandomGenerator):
        # rows first, then columns: the order of the draws is part of the contract
        target_vert_offset, original_up, original_down = cls.sample_cropping_positions_along_axis(
            core_size=core_size, pad_size=pad_size, crop_size=crop_size, length=height, rng=rng)
        target_hori_offset, original_left, original_right = cls.sample_cropping_positions_along_axis(
            core_size=core_size, pad_size=pad_size, crop_size=crop_size, length=width, rng=rng)
        return (target_vert_offset, original_up, original_down, target_hori_offset, original_left, original_right)

    @classmethod
    def create_from_cropping_positions(cls, height: int, width: int, pad_size: int, pad_value: int, core_size: int,
                                       crop_size: int, target_vert_offset: int, original_up: int, original_down: int,
                                       target_hori_offset: int, original_left: int, original_right: int):
        original_box = Box(up=original_up, down=original_down, left=original_left, right=original_right)
        target_box = Box(
            up=target_vert_offset,
            down=target_vert_offset + original_box.height - 1,
            left=target_hori_offset,
            right=target_hori_offset + original_box.width - 1,
        )
        target_core_begin = pad_size
        target_core_end = target_core_begin + core_size - 1
        target_core_box = Box(up=target_core_begin, down=target_core_end, left=target_core_begin,
                              right=target_core_end)
        original_core_box = Box(
            up=original_up + target_core_box.up - target_box.up,
            down=original_down + target_core_box.down - target_box.down,
            left=original_left + target_core_box.left - target_box.left,
            right=original_right + target_core_box.right - target_box.right,
        )
        return CropperState(height=height, width=width, pad_value=pad_value, crop_size=crop_size,
                            original_box=original_box, target_box=target_box, target_core_box=target_core_box,
                            original_core_box=original_core_box)

    @classmethod
    def create_from_random_proposal(cls, shape: Tuple[int, int], core_size: int, pad_size: int, pad_value: int,
                                    rng: RandomGenerator):
        height, width = shape
        crop_size = 2 * pad_size + core_size
        positions = cls.sample_cropping_positions(height=height, width=width, core_size=core_size, pad_size=pad_size,
                                                  crop_size=crop_size, rng=rng)
        return cls.create_from_cropping_positions(height, width, pad_size, pad_value, core_size, crop_size, *positions)

    @classmethod
    def create_from_center_point(cls, shape: Tuple[int, int], core_size: int, pad_size: int, pad_value: int,
                                 center_point: Point):
        height, width = shape
        crop_size = 2 * pad_size + core_size

        assert 0 <= center_point.y < height
        assert 0 <= center_point.x < width

        target_vert_offset = 0
        up = center_point.y - crop_size // 2
        down = up + crop_size - 1
        if up < 0:
            target_vert_offset = abs(up)
            up = 0
        down = min(height - 1, down)

        target_hori_offset = 0
        left = center_point.x - crop_size // 2
        right = left + crop_size - 1
        if left < 0:
            target_hori_offset = abs(left)
            left = 0
        right = min(width - 1, right)

        return CropperState.create_from_cropping_positions(height, width, pad_size, pad_value, core_size, crop_size,
                                                           target_vert_offset, up, down, target_hori_offset, left,
                                                           right)

    @property
    def need_post_filling(self):
        return self.original_box.height != self.crop_size or self.original_box.width != self.crop_size

    @property
    def cropped_shape(self):
        return (self.crop_size,) * 2

    @property
    def pad_size(self):
        return self.target_core_box.up

    @property
    def core_size(self):
        return self.target_core_box.height

    def to_crop_window(self):
        """The ``vkx_crop_window`` of this crop: (up, left, height, width) of original_box, target_box's origin."""
        box = self.original_box
        return (box.up, box.left, box.height, box.width, self.target_box.up, self.target_box.left)


def run_crop_planes(jobs, windows, page_shape, core_size, pad_size, factor=0):
    """``_native.crop_planes`` for element planes that may live on the host: host sources are uploaded (to the context of
    the first device source, or the default one) and every output of a job whose source was on the host comes back as numpy."""
    ctx = next((job['src'].ctx for job in jobs if isinstance(job['src'], _native.DevArray)), None) or _native.default_ctx()
    host = [not isinstance(job['src'], _native.DevArray) for job in jobs]
    uploaded = {}
    for job in jobs:
        src = job['src']
        if not isinstance(src, _native.DevArray):
            key = id(src)
            if key not in uploaded:
                uploaded[key] = (ctx.to_device(src), src)      # (the pair keeps `src` alive while its id is a key)
            job['src'] = uploaded[key][0]
        elif src.ctx is not ctx:
            src.ctx.sync()
            job['src'] = _native.device_copy(src, ctx)
    outs = _native.crop_planes(jobs, windows, page_shape, core_size, pad_size, factor)
    return [tuple(None if a is None else (a.host() if on_host else a) for a in pair) for pair, on_host in zip(outs, host)]


class Cropper:

    @classmethod
    def create_from_random_proposal(cls, shape: Tuple[int, int], core_size: int, pad_size: int, rng: RandomGenerator,
                                    pad_value: int = 0):
        return Cropper(CropperState.create_from_random_proposal(shape=shape, core_size=core_size, pad_size=pad_size,
                                                                pad_value=pad_value, rng=rng))

    @classmethod
    def create_from_center_point(cls, shape: Tuple[int, int], core_size: int, pad_size: int, center_point: Point,
                                 pad_value: int = 0):
        return Cropper(CropperState.create_from_center_point(shape=shape, core_size=core_size, pad_size=pad_size,
                                                             pad_value=pad_value, center_point=center_point))

    def __init__(self, cropper_state: CropperState):
        self.cropper_state = cropper_state

    @property
    def original_box(self):
        return self.cropper_state.original_box

    @property
    def target_box(self):
        return self.cropper_state.target_box

    @property
    def target_core_box(self):
        return self.cropper_state.target_core_box

    @property
    def original_core_box(self):
        return self.cropper_state.original_core_box

    @property
    def need_post_filling(self):
        return self.cropper_state.need_post_filling

    @property
    def crop_size(self):
        return self.cropper_state.crop_size

    @property
    def cropped_shape(self):
        return self.cropper_state.cropped_shape

    @property
    def pad_value(self):
        return self.cropper_state.pad_value

    def _crop(self, element, core_only, fill=0):
        state = self.cropper_state
        assert element.box is None and element.shape == (state.height, state.width)
        (out, _), = run_crop_planes([dict(src=element.arr, window=0, core_only=core_only, fill=fill)], [state.to_crop_window()],
                                    element.shape, state.core_size, state.pad_size)
        return out

    def crop_mask(self, mask: Mask, core_only: bool = False):
        cropped = Mask(mat=self._crop(mask, core_only))
        return cropped.to_box_attached(self.target_core_box) if core_only else cropped

    def crop_score_map(self, score_map: ScoreMap, core_only: bool = False):
        cropped = ScoreMap(mat=self._crop(score_map, core_only), is_prob=score_map.is_prob)
        return cropped.to_box_attached(self.target_core_box) if core_only else cropped

    def crop_image(self, image: Image):
        return Image(mat=self._crop(image, False, fill=self.pad_value))
