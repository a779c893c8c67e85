"""The external_ellipse char-mask engine (reference: engine/char_mask/external_ellipse.py): each char is labelled with the
disc around its inscribed square, warped into the char's perspective.  All chars of a call are rasterised on the device by
vkx_char_mask_ellipse_sets_fresh_dev (csrc/char_mask.hip): three launches and one synchronisation, whatever the char count.

The exceptions the reference raises for a char -- a disc wholly outside the page or bounding box (RuntimeError from the
Mask constructor), a quad that collapses (AssertionError from Box.extract_np_array), a non-finite or oversized geometry
(ValueError / OverflowError from math.ceil) -- are raised here for the first such char, and then no plane is returned."""
from typing import List, Optional, Sequence

import attrs
import numpy as np
from numpy.random import Generator as RandomGenerator

from vkit_amd import _native
from vkit_amd.element import Box, Mask, PolygonSoup
from .type import CharMask, CharMaskEngineRunConfig


@attrs.define
class CharMaskExternalEllipseEngineInitConfig:
    internal_side_length: int = 40


_STATUS_ERRORS = {
    1: lambda: RuntimeError('self.shape != box.shape.'),
    2: lambda: AssertionError(),
    3: lambda: ValueError('cannot convert float NaN to integer'),
    4: lambda: OverflowError('cannot convert float infinity to integer'),
}


def char_quads(char_polygons) -> np.ndarray:
    """float64 (N, 4, 2) smooth (x, y) of the chars; AssertionError for a char without exactly 4 points (reference :133)."""
    if isinstance(char_polygons, PolygonSoup):
        if len(char_polygons) and not (np.diff(char_polygons.offsets) == 4).all():
            raise AssertionError()
        return char_polygons.smooth_xy.reshape(-1, 4, 2)
    quads = []
    for polygon in char_polygons:
        xy = np.asarray(polygon.smooth_xy, dtype=np.float64).reshape(-1, 2)
        if xy.shape[0] != 4:
            raise AssertionError()
        quads.append(xy)
    return np.stack(quads) if quads else np.zeros((0, 4, 2), np.float64)


def raise_for_statuses(sets: Sequence[_native.CharMaskSet]):
    """The reference's exception for the first char that has one, sets in the order the reference runs them."""
    for s in sets:
        bad = np.nonzero(s.boxes[:, 4] != 0)[0]
        if bad.size:
            raise _STATUS_ERRORS.get(int(s.boxes[bad[0], 4]), lambda: RuntimeError('char mask geometry'))()
    raise RuntimeError('char mask call failed without a char status')


def new_planes(shape, want_mask: bool, want_score: bool):
    """Fresh (uninitialised) planes where the page lives: DevArrays in resident mode, numpy arrays otherwise."""
    if _native.resident_mode():
        ctx = _native.default_ctx()
        return (ctx.dev_empty(shape, np.uint8) if want_mask else None, ctx.dev_empty(shape, np.float32) if want_score else None)
    return (np.empty(shape, np.uint8) if want_mask else None, np.empty(shape, np.float32) if want_score else None)


class CharMaskExternalEllipseEngine:

    @classmethod
    def get_type_name(cls) -> str:
        return 'external_ellipse'

    def __init__(self, init_config: CharMaskExternalEllipseEngineInitConfig, init_resource=None):
        self.init_config = init_config
        if not 1 <= int(init_config.internal_side_length) <= 2048:
            raise ValueError('internal_side_length must be in 1 .. 2048')

    def run(self, run_config: CharMaskEngineRunConfig, rng: Optional[RandomGenerator] = None) -> CharMask:
        char_polygons = run_config.char_polygons
        char_bounding_boxes = run_config.char_bounding_boxes
        if run_config.char_bounding_polygons:
            raise NotImplementedError('char_bounding_polygons is outside the accelerated path')
        shape = (run_config.height, run_config.width)
        bounds = None
        if char_bounding_boxes:
            assert len(char_bounding_boxes) == len(char_polygons)
            bounds = np.asarray([(b.up, b.down, b.left, b.right) for b in char_bounding_boxes], np.int32).reshape(-1, 4)
            if bounds.size and not ((bounds[:, 0] >= 0) & (bounds[:, 0] <= bounds[:, 1]) & (bounds[:, 1] < shape[0]) &
                                    (bounds[:, 2] >= 0) & (bounds[:, 2] <= bounds[:, 3]) & (bounds[:, 3] < shape[1])).all():
                raise ValueError('char bounding boxes must lie inside the page')
        mask, _ = new_planes(shape, True, False)
        char_set = _native.CharMaskSet(char_quads(char_polygons), bounds=bounds, mask=mask, want_char_masks=True)
        if not _native.char_mask_ellipse_sets(self.init_config.internal_side_length, [char_set], shape):
            raise_for_statuses([char_set])
        char_masks: List[Mask] = []
        at = 0
        for up, down, left, right, _status in char_set.boxes.tolist():
            bh, bw = down - up + 1, right - left + 1
            view = char_set.char_masks[at:at + bh * bw].reshape(bh, bw)
            at += bh * bw
            char_masks.append(Mask(mat=view, box=Box(up=up, down=down, left=left, right=right)))
        return CharMask(combined_chars_mask=Mask(mat=mask), char_masks=char_masks)
