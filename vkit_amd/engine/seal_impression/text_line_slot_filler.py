"""``fill_text_line_to_seal_impression`` (reference: vkit/engine/seal_impression/text_line_slot_filler.py:28-205): the chars of
curved text lines rotated into the char slots of a seal impression, the internal text line, and the rescale to the seal's alpha.

The host keeps what is a handful of numbers a char: the slot lookup and the two "something wrong" breaks, the resized width and
the char polygon, the ``RotateState`` of ``char_slot.angle - 270`` (the ``rotate`` operator's own host half: matrix, size, point
and polygon, unclipped), the destination box from ``point_up`` with the out-of-bound skip, and the internal text line's shift
and char polygons.  Every pixel is the device's: ``vkx_seal_fill_dev`` resizes every glyph, rotates every char plane, keeps the
maximum, lays the internal line over it and rescales, for ALL seals of a page in three launches
(``fill_text_lines_to_seal_impressions``); host glyph arrays travel with the records as one staged block.

A glyph without a score map goes the mask way.  Where its mask has to be resized the reference stops at an ``assert`` of
``Mask.to_resized_mask`` (the mask ``get_glyph_mask`` returns is attached to the char box); here, as under ``python -O`` there,
the mask is resized: ``(mask * 255)`` in uint8 arithmetic, ``> 0``."""
import logging
from typing import List, Optional, Sequence, Tuple

import attrs
import numpy as np

from vkit_amd import _native
from vkit_amd.element import Point, Polygon, ScoreMap
from vkit_amd.mechanism.distortion import rotate

logger = logging.getLogger(__name__)


class _HostPlanes:
    """The host arrays of a call, each once, packed into the block that travels with the records."""

    def __init__(self):
        self.parts, self.offsets, self.size = [], {}, 0

    def add(self, array: np.ndarray):
        key = id(array)
        if key not in self.offsets:
            flat = np.ascontiguousarray(array)
            self.offsets[key] = (self.size, flat)          # (the array stays alive: its id stays its own)
            self.parts.append((self.size, flat))
            self.size += -(-flat.nbytes // 16) * 16
        return self.offsets[key][0]

    def block(self):
        out = np.zeros(self.size, np.uint8)
        for offset, flat in self.parts:
            out[offset:offset + flat.nbytes] = flat.reshape(-1).view(np.uint8)
        return out


def _source(arr, planes: _HostPlanes, keep: list):
    """(address, row step in bytes, kind) of a float32 plane or a uint8 plane of 1 or 3 channels, on the host or the device."""
    if arr.dtype == np.float32 and arr.ndim == 2:
        kind, row = _native.SEAL_SRC_F32, arr.shape[1] * 4
    elif arr.dtype == np.uint8 and arr.ndim == 2:
        kind, row = _native.SEAL_SRC_U8C1, arr.shape[1]
    elif arr.dtype == np.uint8 and arr.ndim == 3 and arr.shape[2] in (1, 3):
        kind, row = (_native.SEAL_SRC_U8C1 if arr.shape[2] == 1 else _native.SEAL_SRC_U8C3), arr.shape[1] * arr.shape[2]
    else:
        raise NotImplementedError(f'glyph plane of dtype {arr.dtype} and shape {tuple(arr.shape)}')
    if isinstance(arr, np.ndarray):
        return planes.add(arr), row, kind | _native.SEAL_SRC_HOST
    keep.append(arr)
    return arr.ptr, row, kind


def _seal_chars(seal_index, seal_impression, text_line_slot_indices, text_lines, planes, keep, records, char_polygons):
    """The char records of one seal (reference :39-179), appended to ``records``; the placed chars' polygons to ``char_polygons``."""
    height, width = seal_impression.shape
    assert len(text_line_slot_indices) == len(text_lines)
    for text_line_slot_idx, text_line in zip(text_line_slot_indices, text_lines):
        if text_line_slot_idx >= len(seal_impression.text_line_slots):
            logger.error('fill_text_line_to_seal_impression: something wrong.')
            break
        assert text_line.is_hori
        assert not text_line.shifted
        text_line_slot = seal_impression.text_line_slots[text_line_slot_idx]

        # the tallest reference char of the line sets the aspect ratio the slot's is compared with
        text_line_ref_char_height = 0
        text_line_ref_char_width = 0
        for char_glyph in text_line.char_glyphs:
            if char_glyph.ref_char_height > text_line_ref_char_height:
                text_line_ref_char_height = char_glyph.ref_char_height
                text_line_ref_char_width = char_glyph.ref_char_width
        assert text_line_ref_char_height > 0 and text_line_ref_char_width > 0
        text_line_aspect_ratio = text_line_ref_char_width / text_line_ref_char_height
        resized_char_width_factor = text_line_slot.char_aspect_ratio / text_line_aspect_ratio
        plane_height = text_line.box.height

        for char_slot_idx, (char_box, char_glyph) in enumerate(zip(text_line.char_boxes, text_line.char_glyphs)):
            if char_slot_idx >= len(text_line_slot.char_slots):
                logger.error('fill_text_line_to_seal_impression: something wrong.')
                break
            char_slot = text_line_slot.char_slots[char_slot_idx]

            # only the width of a char is resized; its rows keep their place in the text line's height
            resized_width = max(1, round(resized_char_width_factor * char_glyph.width))
            resized_box = attrs.evolve(char_box.box, left=0, right=resized_width - 1)
            if resized_box.up < 0 or resized_box.down >= plane_height:
                raise ValueError('char box outside the height of its text line')
            if char_glyph.score_map:
                source = char_glyph.score_map.arr
            else:
                # LCD, fallback to mask: any(image > 0), formed by the kernel
                source = char_glyph.image.arr
                assert tuple(source.shape[:2]) == char_box.box.shape      # get_glyph_mask(box=...) without enable_resize
            address, step, kind = _source(source, planes, keep)

            # the char polygon, widened to the (resized) reference char
            up, down = resized_box.up, resized_box.down
            ref_char_height = char_glyph.ref_char_height
            if resized_box.height < ref_char_height:
                half_inc = (ref_char_height - resized_box.height) / 2
                up, down = up - half_inc, down + half_inc
            left, right = resized_box.left, resized_box.right
            ref_char_width = resized_char_width_factor * char_glyph.ref_char_width
            if resized_box.width < ref_char_width:
                half_inc = (ref_char_width - resized_box.width) / 2
                left, right = left - half_inc, right + half_inc
            char_polygon = Polygon.from_xy_pairs([(left, up), (right, up), (right, down), (left, down)])

            # horizontal text line has angle 270; the char polygon could be out-of-bound and is not clipped
            angle = char_slot.angle - 270
            rotated = rotate.distort({'angle': angle}, (plane_height, resized_width), point=Point.create(y=0, x=resized_width / 2),
                                     polygon=char_polygon, disable_clip_result_elements=True, get_state=True)
            rotated_height, rotated_width = rotated.shape
            assert rotated.point and rotated.polygon

            # the bounding box from point_up: the rotated point's position is the offset
            dst_up = char_slot.point_up.y - rotated.point.y
            dst_down = dst_up + rotated_height - 1
            dst_left = char_slot.point_up.x - rotated.point.x
            dst_right = dst_left + rotated_width - 1
            if dst_up < 0 or dst_down >= height or dst_left < 0 or dst_right >= width:
                logger.error('fill_text_line_to_seal_impression: out-of-bound.')
                continue

            record = np.zeros((), _native.SEAL_CHAR_DTYPE)
            record['src'], record['src_step'], record['src_kind'] = address, step, kind
            record['src_h'], record['src_w'] = source.shape[:2]
            record['glyph_h'], record['glyph_up'] = resized_box.height, resized_box.up
            record['interpolation'] = text_line.cv_resize_interpolation
            record['plane_h'], record['plane_w'] = plane_height, resized_width
            record['identity'] = int(angle == 0)
            record['m'] = np.asarray(rotated.state.trans_mat, np.float32).reshape(6)
            record['rot_h'], record['rot_w'] = rotated_height, rotated_width
            record['seal'], record['dst_up'], record['dst_left'] = seal_index, dst_up, dst_left
            records.append(record)
            char_polygons.append(rotated.polygon.to_shifted_polygon(offset_y=dst_up, offset_x=dst_left))


def build_seal_fill_tables(items: Sequence[Tuple]):
    """The host half of a call: ``(chars, seals, planes_host, keep, polygons, floats)`` -- the SEAL_CHAR_DTYPE and SEAL_REC_DTYPE
    tables of ``vkx_seal_fill_dev``, the block of host planes they address, the device arrays they address (to be kept alive until
    the call is queued), the char polygons of every seal and the length of the packed destination."""
    planes, keep, records = _HostPlanes(), [], []
    seals = np.zeros(len(items), _native.SEAL_REC_DTYPE)
    polygons: List[List[Polygon]] = []
    offset = 0
    for index, (seal_impression, text_line_slot_indices, text_lines, internal_text_line) in enumerate(items):
        height, width = seal_impression.shape
        char_polygons: List[Polygon] = []
        _seal_chars(index, seal_impression, text_line_slot_indices, text_lines, planes, keep, records, char_polygons)
        seal = seals[index]
        seal['h'], seal['w'], seal['dst_off'], seal['alpha'] = height, width, offset, seal_impression.alpha
        seal['internal_kind'] = _native.SEAL_INTERNAL_NONE
        if internal_text_line:
            internal_text_line_box = seal_impression.internal_text_line_box
            assert internal_text_line_box
            # (marks the CALLER's internal text line as shifted, as the reference's to_shifted_text_line does)
            internal_text_line = internal_text_line.to_shifted_text_line(offset_y=internal_text_line_box.up,
                                                                         offset_x=internal_text_line_box.left)
            # a plain overwrite of its box, applied after all chars
            source = internal_text_line.score_map.arr if internal_text_line.score_map else internal_text_line.mask.arr
            box = internal_text_line.box
            assert tuple(source.shape) == box.shape
            seal['internal'], seal['internal_step'], seal['internal_kind'] = _source(source, planes, keep)
            seal['internal_up'], seal['internal_left'], seal['internal_h'], seal['internal_w'] = box.up, box.left, box.height, box.width
            char_polygons.extend(internal_text_line.to_char_polygons(page_height=height, page_width=width))
        polygons.append(char_polygons)
        offset += height * width
    chars = np.array(records, _native.SEAL_CHAR_DTYPE) if records else np.zeros(0, _native.SEAL_CHAR_DTYPE)
    return chars, seals, planes.block(), keep, polygons, offset


def fill_text_lines_to_seal_impressions(items: Sequence[Tuple]) -> List[Tuple[ScoreMap, List[Polygon]]]:
    """``fill_text_line_to_seal_impression`` for every ``(seal_impression, text_line_slot_indices, text_lines,
    internal_text_line)`` of ``items`` in ONE device call: ``[(score_map, char_polygons), ...]`` in their order.  Inside
    ``_native.resident(True)`` the score maps stay on the device (views of one packed array); otherwise they are host arrays."""
    if not items:
        return []
    chars, seals, planes_host, keep, polygons, floats = build_seal_fill_tables(items)
    dst = _native.default_ctx().dev_empty((floats,), np.float32)
    _native.seal_fill(chars, seals, dst, planes_host)
    del keep

    resident = _native.resident_mode()
    host = None if resident else dst.host()
    results = []
    for seal, char_polygons in zip(seals, polygons):
        shape, at = (int(seal['h']), int(seal['w'])), int(seal['dst_off'])
        if resident:
            mat = _native.DevView(dst, at * 4, shape, np.float32)
        else:
            mat = np.array(host[at:at + shape[0] * shape[1]]).reshape(shape)
        # (ScoreMap.assign_mat in the reference: the rescaled map is not checked, an all-zero seal is NaN throughout)
        results.append((ScoreMap.from_unchecked_mat(mat), char_polygons))
    return results


def fill_text_line_to_seal_impression(seal_impression, text_line_slot_indices: Sequence[int], text_lines: Sequence,
                                      internal_text_line: Optional[object]):
    """The text-line score map of one seal impression and the polygons of its placed chars: ``(score_map, char_polygons)``."""
    return fill_text_lines_to_seal_impressions([(seal_impression, text_line_slot_indices, text_lines, internal_text_line)])[0]
