"""The pixel half of the reference's PageTextRegionStep (vkit/pipeline/text_detection/page_text_region.py) and the step's
output container.

``PageTextRegionStepOutput`` (:177-186) is the input of PageTextRegionLabelStep and PageTextRegionCroppingStep.  The step as
a whole needs rectpack and pyclipper and stays outside the accelerated path; what is here is
everything of it that is pixel work, batched over all text regions of a page (csrc/region_masks.hip,
csrc/region_flatten.hip, csrc/contours.hip, csrc/polygon_overlap.hip):

* ``PageTextRegionStep.generate_precise_text_region_candidate_polygons`` (:868-897) and its plural form: the AND of a precise
  mask and a disconnected text-region mask over their common box, then the outer contours (``Mask.to_disconnected_polygons``,
  cv.findContours on the device) -- eight launches and one synchronisation for all pairs of a list;
* ``calculate_boxed_masks_intersected_ratio`` (:189-227), ``PageTextRegionStep.strtree_query_intersected_polygons`` (:899-925)
  and the binding of the page's chars to its precise text regions (:1160-1216: ``intersected_polygon_ratios``,
  ``bind_char_polygons``, ``build_page_text_region_infos``), with ``find_precise_text_region_candidate_polygons`` (:1115-1149)
  composed on top: the STR-tree query is the closed integer envelope test (``envelope_pairs``, no shapely), every polygon
  is rasterised once into a bit plane and every pair is counted -- three launches, one copy-out and one synchronisation
  whatever the numbers of chars and regions; the ratios are formed on the host from the integer counts;
* ``TextRegionFlattener.get_bounding_extended_text_region_masks`` (:477-558): the page's text mask by the fresh mask paint,
  then the three rasters and the mask algebra of every region -- three launches, no synchronisation while no polygon has
  more than 64 vertices;
* ``TextRegionFlattener.build_flattened_text_regions`` (:560-656): cut, rotate and trim every region -- three launches and
  one synchronisation (the read of the rotated masks' extents) whatever the number of regions;
* ``resize_flattened_text_regions`` / ``post_rotate_flattened_text_regions``, the batched forms of
  ``FlattenedTextRegion.to_resized_flattened_text_region`` and ``.to_post_rotated_flattened_text_region`` (:109-166): one
  launch each, no synchronisation;
* ``build_background_image_for_stacking`` and ``stack_flattened_text_regions`` (:732-856): one launch, no synchronisation.

The polygon geometry that decides the polygons and the angles (shapely, pyclipper, the KD-tree) is the caller's
(the host's); the masks built from them flow into the flattening on the device.  Results are device resident inside
``_native.resident(True)`` or when an input was; otherwise they come back as numpy arrays, by one copy a call.
"""
import logging
import math
import statistics
from typing import Any, List, Optional, Sequence, Tuple

import attrs
import numpy as np

from vkit_amd import _native
from vkit_amd.element import Box, Image, Mask, Polygon
from vkit_amd.mechanism.distortion.geometric.affine import RotateConfig, RotateState, rotate

logger = logging.getLogger(__name__)


@attrs.define
class PageTextRegionStepOutput:
    page_image: Image
    page_active_mask: Mask
    page_char_polygons: Sequence[Polygon]
    page_text_region_polygons: Sequence[Polygon]
    page_char_polygon_text_region_polygon_indices: Sequence[int]
    shape_before_rotate: Tuple[int, int]
    rotate_angle: int
    debug: Optional[Any]


_UNSET = object()


@attrs.define
class FlattenedTextRegion:
    is_typical: bool
    text_region_polygon: Polygon
    bounding_extended_text_region_mask: Mask
    flattening_rotate_angle: int
    shape_before_trim: Tuple[int, int]
    rotated_trimmed_box: Box
    shape_before_resize: Tuple[int, int]
    post_rotate_angle: int
    flattened_image: Image
    flattened_mask: Mask
    flattened_char_polygons: Optional[Sequence[Polygon]]
    # the reference's field ``text_region_image``: ``bounding_extended_text_region_mask.extract_image(page image)``, made on
    # first access (the flattening itself reads the page under the mask inside its warp kernel)
    _text_region_image: Any = attrs.field(default=_UNSET, alias='text_region_image', repr=False)
    _page_image: Optional[Image] = attrs.field(default=None, alias='page_image', repr=False, eq=False)

    @property
    def text_region_image(self) -> Image:
        if self._text_region_image is _UNSET:
            assert self._page_image is not None
            self._text_region_image = self.bounding_extended_text_region_mask.extract_image(self._page_image)
        return self._text_region_image

    @property
    def shape(self):
        return self.flattened_image.shape

    @property
    def height(self):
        return self.flattened_image.height

    @property
    def width(self):
        return self.flattened_image.width

    @property
    def area(self):
        return self.flattened_image.area

    def get_char_height_meidan(self):
        assert self.flattened_char_polygons
        return statistics.median(
            char_polygon.get_rectangular_height() for char_polygon in self.flattened_char_polygons)

    def to_resized_flattened_text_region(self, resized_height: Optional[int] = None, resized_width: Optional[int] = None):
        return resize_flattened_text_regions([self], [(resized_height, resized_width)])[0]

    def to_post_rotated_flattened_text_region(self, post_rotate_angle: int):
        assert self.post_rotate_angle == 0
        return _rotate_flattened_text_regions([self], [post_rotate_angle])[0]


# ---- planes of a batched call: where they come from, where they go -------------------------------------------------
class _Sources:
    """The source planes of one batched call as device pointers: device arrays are used where they are, host arrays are
    packed and uploaded by one copy."""

    def __init__(self, arrays):
        owners = [a.ctx for a in arrays if isinstance(a, _native.DevArray)]
        self.ctx = owners[0] if owners else _native.default_ctx()
        for ctx in owners:
            if ctx is not self.ctx:
                ctx.sync()
        self.resident = _native.resident_mode() or bool(owners)
        self.ptr = [0] * len(arrays)
        host = [(k, np.ascontiguousarray(a)) for k, a in enumerate(arrays) if not isinstance(a, _native.DevArray)]
        offsets, total = _layout([a.nbytes for _, a in host])
        self.keep = [a for a in arrays if isinstance(a, _native.DevArray)]
        if host:
            packed = np.empty(total, np.uint8)
            for (_, a), off in zip(host, offsets):
                packed[off:off + a.nbytes] = a.reshape(-1).view(np.uint8)
            block = self.ctx.to_device(packed)
            self.keep.append(block)
            for (k, _), off in zip(host, offsets):
                self.ptr[k] = block.ptr + off
        for k, a in enumerate(arrays):
            if isinstance(a, _native.DevArray):
                self.ptr[k] = a.ptr


def _layout(sizes):
    offsets, total = [], 0
    for size in sizes:
        offsets.append(total)
        total += (int(size) + 255) & ~255
    return offsets, max(total, 256)


class _Packed:
    """The packed destination of one batched call and the planes cut out of it (device views, or numpy views of its one
    download)."""

    def __init__(self, ctx, shapes, resident):
        self.shapes = [tuple(int(v) for v in s) for s in shapes]
        self.offsets, total = _layout([math.prod(s) for s in self.shapes])
        self.dev = ctx.dev_empty((total,), np.uint8)
        self.resident = resident
        self._host = None

    def plane(self, k):
        off, shape = self.offsets[k], self.shapes[k]
        if self.resident:
            return _native.DevView(self.dev, off, shape)
        if self._host is None:
            self._host = np.array(self.dev.host())
        return self._host[off:off + math.prod(shape)].reshape(shape)


def _arr(element):
    arr = element.arr
    if np.dtype(arr.dtype) != np.uint8:
        raise TypeError('uint8 planes only')
    return arr


def _check_image(arr):
    if arr.ndim != 3 or arr.shape[2] != 3:
        raise ValueError('the pixel half of PageTextRegionStep takes RGB images (height, width, 3)')


def _rotate_state(angle, shape):
    config = RotateConfig(angle=angle)
    return config, RotateState(config, shape, None)


def _rotate_polygons(config, shape, polygons):
    """the polygons of rotate.distort on the host (the existing affine_polygons path, clipped to the result shape)"""
    return rotate.distort(config, shapable_or_shape=shape, polygons=polygons).polygons


# ---- TextRegionFlattener -----------------------------------------------------------------------------------------
class TextRegionFlattener:
    """``get_bounding_extended_text_region_masks`` (:477-558) and ``build_flattened_text_regions`` (:560-656) of the
    reference's class.  The geometric methods that lead to their arguments (polygon dilation, minimum-area rectangles, the
    KD-tree of the main angles) are the caller's."""

    @classmethod
    def get_bounding_extended_text_region_masks(cls, shape: Tuple[int, int], text_region_polygons: Sequence[Polygon],
                                                dilated_text_region_polygons: Sequence[Polygon],
                                                bounding_rectangular_polygons: Sequence[Polygon],
                                                typical_indices: Sequence[int], main_angles: Sequence[int]):
        """One box-attached mask a text region: the (possibly dilated) region trimmed by the other text regions under its
        bounding rectangle, united with the non-text part of that rectangle.  Device views inside ``_native.resident(True)``,
        numpy arrays from one download otherwise."""
        typical_indices_set = set(typical_indices)
        n = len(text_region_polygons)
        if n == 0:
            return []
        ctx = _native.default_ctx()
        height, width = (int(v) for v in shape)

        # the text mask of the page: every text-region polygon, painted into a fresh device plane
        text_mask = ctx.dev_empty((height, width), np.uint8)
        originals = [polygon.to_np_array() for polygon in text_region_polygons]
        _native.paint_polys(originals, mask=text_mask, fresh=True)

        boxes: List[Box] = []
        tables = []
        records = np.zeros(n, _native.REGION_MASKS_REC_DTYPE)
        at = 0
        for idx in range(n):
            dilated_text_region_polygon = dilated_text_region_polygons[idx]
            bounding_rectangular_polygon = bounding_rectangular_polygons[idx]
            if typical_indices_set and idx not in typical_indices_set:
                # Patch bounding rectangular polygon if is nontypical.
                bounding_rectangular_polygon = dilated_text_region_polygon.to_bounding_rectangular_polygon(
                    shape=shape, angle=main_angles[idx])
            # (the rectangle may leave the dilated polygon's box a little: the union of the two)
            box = Box.from_boxes((dilated_text_region_polygon.bounding_box, bounding_rectangular_polygon.bounding_box))
            boxes.append(box)
            rec = records[idx]
            rec['up'], rec['down'], rec['left'], rec['right'] = box.up, box.down, box.left, box.right
            for name, points in (('o', originals[idx]), ('d', dilated_text_region_polygon.to_np_array()),
                                 ('r', bounding_rectangular_polygon.to_np_array())):
                rec[name + '_off'], rec[name + '_cnt'] = at, len(points)
                tables.append(points)
                at += len(points)
        out = _Packed(ctx, [box.shape for box in boxes], _native.resident_mode())
        records['dst_off'] = out.offsets
        _native.region_extend_masks(records, np.concatenate(tables, axis=0), text_mask, out.dev)
        return [Mask(mat=out.plane(k), box=box) for k, box in enumerate(boxes)]

    @classmethod
    def build_flattened_text_regions(cls, image: Image, text_region_polygons: Sequence[Polygon],
                                     bounding_extended_text_region_masks: Sequence[Mask], typical_indices: Sequence[int],
                                     flattening_rotate_angles: Sequence[int],
                                     grouped_char_polygons: Optional[Sequence[Sequence[Polygon]]]):
        typical_indices_set = set(typical_indices)
        # (the reference zips the three sequences: the shortest decides)
        n = min(len(text_region_polygons), len(bounding_extended_text_region_masks), len(flattening_rotate_angles))
        if n == 0:
            return []
        page = _arr(image)
        _check_image(page)
        masks = list(bounding_extended_text_region_masks[:n])
        src = _Sources([page] + [_arr(m) for m in masks])
        ctx = src.ctx
        page_h, page_w = page.shape[:2]

        states, boxes = [], []
        for mask, angle in zip(masks, flattening_rotate_angles):
            box = mask.box
            assert box
            assert 0 <= box.up and box.down < page_h and 0 <= box.left and box.right < page_w
            boxes.append(box)
            states.append(_rotate_state(angle, box.shape))

        # launch 1: the rotated masks, whole; launch 2: their extents; the one synchronisation: the extents on the host
        full = _Packed(ctx, [(s.dsize[1], s.dsize[0]) for _, s in states], True)
        pairs = np.zeros(n, _native.REGION_WARP_PAIR_DTYPE)
        for k, (box, (_, state)) in enumerate(zip(boxes, states)):
            p = pairs[k]
            p['src_image'] = src.ptr[0] + (box.up * page_w + box.left) * 3
            p['src_image_step'] = page_w * 3
            p['src_mask'], p['src_mask_step'] = src.ptr[1 + k], box.width
            p['src_h'], p['src_w'] = box.height, box.width
            p['m'] = state.trans_mat.reshape(6)
            p['dst_h'], p['dst_w'] = full.shapes[k]
            p['dst_image_off'], p['dst_mask_off'] = -1, full.offsets[k]
        _native.region_warp(pairs, True, full.dev)
        extents_dev = _native.region_extent(full.dev, full.offsets, full.shapes)
        extents = ctx.pinned_empty((n, 4), np.int32)
        ctx.copy_out(extents_dev.ptr, extents)
        ctx.sync()
        if (extents[:, 0] < 0).any():
            raise RuntimeError('to_external_box: empty np_mask.')

        # launch 3: image and mask again, only the trimmed windows.  Image.to_cropped_image takes `down or height - 1` (and
        # `right or width - 1`): a box that ends in row or column 0 leaves the image untrimmed on that axis while the mask
        # is trimmed, so the two windows of a region can differ; such a region takes two records.
        records, shapes, slots = [], [], []
        for k in range(n):
            up, down, left, right = (int(v) for v in extents[k])
            full_h, full_w = full.shapes[k]
            image_down, image_right = down or full_h - 1, right or full_w - 1
            mask_shape = (down - up + 1, right - left + 1)
            image_shape = (image_down - up + 1, image_right - left + 1)
            shapes += [image_shape + (3,), mask_shape]
            if image_shape == mask_shape:
                records.append((k, up, left, mask_shape, 2 * k, 2 * k + 1))
            else:
                records.append((k, up, left, image_shape, 2 * k, None))
                records.append((k, up, left, mask_shape, None, 2 * k + 1))
        out = _Packed(ctx, shapes, src.resident)
        trimmed = np.zeros(len(records), _native.REGION_WARP_PAIR_DTYPE)
        for p, (k, up, left, shape, image_slot, mask_slot) in zip(trimmed, records):
            for name in ('src_image', 'src_image_step', 'src_mask', 'src_mask_step', 'src_h', 'src_w', 'm'):
                p[name] = pairs[k][name]
            p['up'], p['left'], p['dst_h'], p['dst_w'] = up, left, shape[0], shape[1]
            p['dst_image_off'] = -1 if image_slot is None else out.offsets[image_slot]
            p['dst_mask_off'] = -1 if mask_slot is None else out.offsets[mask_slot]
        _native.region_warp(trimmed, True, out.dev)

        flattened_text_regions: List[FlattenedTextRegion] = []
        for k in range(n):
            box, (config, state) = boxes[k], states[k]
            up, down, left, right = (int(v) for v in extents[k])
            trimmed_char_polygons = None
            if grouped_char_polygons is not None:
                relative = [polygon.to_relative_polygon(origin_y=box.up, origin_x=box.left)
                            for polygon in grouped_char_polygons[k]]
                rotated = _rotate_polygons(config, box.shape, relative) if relative else None
                if rotated:
                    trimmed_char_polygons = [polygon.to_relative_polygon(origin_y=up, origin_x=left) for polygon in rotated]
            flattened_image = Image(mat=out.plane(2 * k))
            flattened_text_regions.append(FlattenedTextRegion(
                is_typical=(k in typical_indices_set),
                text_region_polygon=text_region_polygons[k],
                page_image=image,
                bounding_extended_text_region_mask=masks[k],
                flattening_rotate_angle=flattening_rotate_angles[k],
                shape_before_trim=full.shapes[k],
                rotated_trimmed_box=Box(up=up, down=down, left=left, right=right),
                shape_before_resize=flattened_image.shape,
                post_rotate_angle=0,
                flattened_image=flattened_image,
                flattened_mask=Mask(mat=out.plane(2 * k + 1)),
                flattened_char_polygons=trimmed_char_polygons,
            ))
        return flattened_text_regions


# ---- the batched region methods ------------------------------------------------------------------------------------
def _region_sources(regions):
    arrays = []
    for region in regions:
        image, mask = _arr(region.flattened_image), _arr(region.flattened_mask)
        _check_image(image)
        assert not region.flattened_mask.box
        arrays += [image, mask]
    return _Sources(arrays)


def resize_flattened_text_regions(flattened_text_regions: Sequence[FlattenedTextRegion],
                                  resized_shapes: Sequence[Tuple[Optional[int], Optional[int]]]):
    """``region.to_resized_flattened_text_region(resized_height, resized_width)`` for every region and its
    ``(resized_height, resized_width)`` of ``resized_shapes``, in one launch."""
    from vkit_amd.element.opt import generate_resized_shape
    regions = list(flattened_text_regions)
    assert len(regions) == len(resized_shapes)
    if not regions:
        return []
    src = _region_sources(regions)
    records, shapes = [], []
    for k, (region, (resized_height, resized_width)) in enumerate(zip(regions, resized_shapes)):
        targets = []
        for element in (region.flattened_image, region.flattened_mask):
            # image and mask are resized by calls of their own, each from its own shape
            targets.append(tuple(generate_resized_shape(height=element.height, width=element.width,
                                                        resized_height=resized_height, resized_width=resized_width)))
        shapes += [targets[0] + (3,), targets[1]]
        same = region.flattened_image.shape == region.flattened_mask.shape and targets[0] == targets[1]
        if same:
            records.append((k, region.flattened_image.shape, targets[0], True, True))
        else:
            records.append((k, region.flattened_image.shape, targets[0], True, False))
            records.append((k, region.flattened_mask.shape, targets[1], False, True))
    out = _Packed(src.ctx, shapes, src.resident)
    pairs = np.zeros(len(records), _native.REGION_RESIZE_PAIR_DTYPE)
    for p, (k, (sh, sw), (dh, dw), with_image, with_mask) in zip(pairs, records):
        p['src_image'], p['src_image_step'] = src.ptr[2 * k], sw * 3
        p['src_mask'], p['src_mask_step'] = src.ptr[2 * k + 1], sw
        p['src_h'], p['src_w'], p['dst_h'], p['dst_w'] = sh, sw, dh, dw
        p['dst_image_off'] = out.offsets[2 * k] if with_image else -1
        p['dst_mask_off'] = out.offsets[2 * k + 1] if with_mask else -1
    _native.region_resize(pairs, out.dev)
    results = []
    for k, (region, (resized_height, resized_width)) in enumerate(zip(regions, resized_shapes)):
        polygons = None
        if region.flattened_char_polygons is not None:
            polygons = [polygon.to_conducted_resized_polygon(region.shape, resized_height=resized_height,
                                                             resized_width=resized_width)
                        for polygon in region.flattened_char_polygons]
        results.append(attrs.evolve(region, flattened_image=Image(mat=out.plane(2 * k)),
                                    flattened_mask=Mask(mat=out.plane(2 * k + 1)), flattened_char_polygons=polygons))
    return results


def _rotate_flattened_text_regions(regions, angles):
    """rotate.distort of image, mask and char polygons of every region by its angle (no trim), in one launch"""
    src = _region_sources(regions)
    states = []
    for region, angle in zip(regions, angles):
        assert region.flattened_image.shape == region.flattened_mask.shape
        states.append(_rotate_state(angle, region.shape))
    shapes = []
    for _, state in states:
        shapes += [(state.dsize[1], state.dsize[0], 3), (state.dsize[1], state.dsize[0])]
    out = _Packed(src.ctx, shapes, src.resident)
    pairs = np.zeros(len(regions), _native.REGION_WARP_PAIR_DTYPE)
    for k, (region, (_, state)) in enumerate(zip(regions, states)):
        p = pairs[k]
        p['src_image'], p['src_image_step'] = src.ptr[2 * k], region.width * 3
        p['src_mask'], p['src_mask_step'] = src.ptr[2 * k + 1], region.width
        p['src_h'], p['src_w'] = region.shape
        p['m'] = state.trans_mat.reshape(6)
        p['dst_h'], p['dst_w'] = shapes[2 * k + 1]
        p['dst_image_off'], p['dst_mask_off'] = out.offsets[2 * k], out.offsets[2 * k + 1]
    _native.region_warp(pairs, False, out.dev)
    results = []
    for k, (region, angle, (config, state)) in enumerate(zip(regions, angles, states)):
        polygons = region.flattened_char_polygons
        if polygons is not None:
            polygons = _rotate_polygons(config, region.shape, polygons) if polygons else polygons
        results.append(attrs.evolve(region, post_rotate_angle=angle, flattened_image=Image(mat=out.plane(2 * k)),
                                    flattened_mask=Mask(mat=out.plane(2 * k + 1)), flattened_char_polygons=polygons))
    return results


def post_rotate_flattened_text_regions(flattened_text_regions: Sequence[FlattenedTextRegion], angles: Sequence[int]):
    """``region.to_post_rotated_flattened_text_region(angle)`` for every region with a non-zero angle, in one launch; a region
    whose angle is 0 is returned as it is."""
    regions = list(flattened_text_regions)
    assert len(regions) == len(angles)
    picked = [k for k, angle in enumerate(angles) if angle != 0]
    for k in picked:
        assert regions[k].post_rotate_angle == 0
    if picked:
        rotated = _rotate_flattened_text_regions([regions[k] for k in picked], [angles[k] for k in picked])
        for k, region in zip(picked, rotated):
            regions[k] = region
    return regions


# ---- char binding: mask-overlap ratios (:189-227, :899-925, :1160-1216) ---------------------------------------------------
@attrs.define
class PageTextRegionInfo:
    precise_text_region_polygon: Polygon
    char_polygons: Sequence[Polygon]


def _boxes_meet(anchor_box: Box, candidate_box: Box):
    return (max(anchor_box.up, candidate_box.up) <= min(anchor_box.down, candidate_box.down)
            and max(anchor_box.left, candidate_box.left) <= min(anchor_box.right, candidate_box.right))


def calculate_boxed_masks_intersected_ratios(pairs, use_candidate_as_base: bool = False):
    """``calculate_boxed_masks_intersected_ratio(anchor_mask, candidate_mask, use_candidate_as_base)`` for every
    (anchor_mask, candidate_mask) pair of ``pairs`` -> a list of floats.  The masks are box attached, host or device
    resident; host planes are uploaded by one copy.  All pairs whose boxes meet go through ONE launch, one copy-out and one
    synchronisation; pairs whose boxes do not meet are 0.0 and, when no boxes meet, the device is not touched.  A zero base
    raises ZeroDivisionError, as the reference's division does."""
    pairs = list(pairs)
    for anchor_mask, candidate_mask in pairs:
        assert anchor_mask.box and candidate_mask.box
    met = [k for k, (anchor_mask, candidate_mask) in enumerate(pairs) if _boxes_meet(anchor_mask.box, candidate_mask.box)]
    ratios = [0.0] * len(pairs)
    if not met:
        return ratios
    src = _Sources([_arr(mask) for k in met for mask in pairs[k]])
    records = np.zeros(len(met), _native.MASK_OVERLAP_REC_DTYPE)
    for rec, n, k in zip(records, range(len(met)), met):
        for name, mask, ptr in (('anchor', pairs[k][0], src.ptr[2 * n]), ('candidate', pairs[k][1], src.ptr[2 * n + 1])):
            box = mask.box
            rec[name], rec[name + '_step'] = ptr, box.width
            rec[name + '_up'], rec[name + '_left'], rec[name + '_h'], rec[name + '_w'] = box.up, box.left, box.height, box.width
    counts_dev = _native.mask_overlap_counts(records, ctx=src.ctx)
    counts = src.ctx.pinned_empty((len(met), 3), np.int64)
    src.ctx.copy_out(counts_dev.ptr, counts)
    src.ctx.sync()
    for k, (intersected_area, anchor_area, candidate_area) in zip(met, counts.tolist()):
        base_area = candidate_area if use_candidate_as_base else anchor_area + candidate_area - intersected_area
        ratios[k] = intersected_area / base_area
    return ratios


def calculate_boxed_masks_intersected_ratio(anchor_mask: Mask, candidate_mask: Mask, use_candidate_as_base: bool = False):
    return calculate_boxed_masks_intersected_ratios([(anchor_mask, candidate_mask)], use_candidate_as_base)[0]


def polygon_overlap_tables(polygons: Sequence[Polygon]):
    """The tables of a batch of polygons, vectorised: (``records`` POLY_OVERLAP_REC_DTYPE with ``Polygon.bounding_box`` and the
    point range of every polygon, ``points`` int32 (N, 2) holding ``Polygon.self_relative_polygon.to_np_array()`` of every
    polygon at its range, ``envelopes`` int64 (n, 4) as (xmin, xmax, ymin, ymax) of the integer ``to_xy_pairs()``)."""
    n = len(polygons)
    records = np.zeros(n, _native.POLY_OVERLAP_REC_DTYPE)
    if n == 0:
        return records, np.zeros((0, 2), np.int32), np.zeros((0, 4), np.int64)
    tables = [polygon.to_np_array() for polygon in polygons]
    count = np.array([len(table) for table in tables], np.int64)
    first = np.concatenate([[0], np.cumsum(count)[:-1]])
    if int(count.sum()) > 0x7fffffff:
        raise ValueError('more than 2^31 - 1 points in one batch')
    xy = np.concatenate(tables, axis=0).astype(np.int32).reshape(-1, 2)
    envelopes = np.empty((n, 4), np.int64)
    envelopes[:, 0::2] = np.minimum.reduceat(xy, first, axis=0)
    envelopes[:, 1::2] = np.maximum.reduceat(xy, first, axis=0)
    # Polygon.bounding_box / self_relative_polygon: the integer positions as float32 (the PointTuple quirk), the box from
    # round() of their minima and maxima, the points rounded after the float minimum is subtracted
    smooth = xy.astype(np.float32)
    low = np.minimum.reduceat(smooth, first, axis=0)
    high = np.maximum.reduceat(smooth, first, axis=0)
    relative = np.rint(smooth - np.repeat(low, count, axis=0)).astype(np.int32)
    low, high = np.rint(low).astype(np.int64), np.rint(high).astype(np.int64)
    if (np.abs(low) > 1 << 30).any() or (high - low >= 1 << 31).any():
        raise ValueError('a polygon beyond the int32 range of the tables')
    records['up'], records['left'] = low[:, 1], low[:, 0]
    records['h'], records['w'] = high[:, 1] - low[:, 1] + 1, high[:, 0] - low[:, 0] + 1
    # PointList.from_np_array drops a closing duplicate of the first point
    last = first + count - 1
    closed = (count > 2) & (relative[first] == relative[last]).all(axis=1)
    records['pts_off'], records['pts_cnt'] = first, count - closed
    return records, relative, envelopes


def envelope_pairs(anchor_envelopes: np.ndarray, candidate_envelopes: np.ndarray):
    """What ``sorted(STRtree(anchors).query(candidate))`` answers for every candidate, without shapely: the anchors whose
    envelope (the closed integer rectangle (xmin, xmax, ymin, ymax) of its points) meets the candidate's; touching envelopes
    count.  -> int32 (k, 2) as (candidate, anchor), candidate-major, anchors ascending."""
    a, c = np.asarray(anchor_envelopes, np.int64).reshape(-1, 4), np.asarray(candidate_envelopes, np.int64).reshape(-1, 4)
    out = []
    # (blocks of candidates: the boolean matrix of a block stays below 16 MB)
    step = max(1, (16 << 20) // max(len(a), 1))
    for at in range(0, len(c), step):
        b = c[at:at + step, None, :]
        meet = (a[None, :, 0] <= b[:, :, 1]) & (b[:, :, 0] <= a[None, :, 1]) & (a[None, :, 2] <= b[:, :, 3]) & (b[:, :, 2] <= a[None, :, 3])
        ci, ai = np.nonzero(meet)
        out.append(np.stack([ci + at, ai], axis=1))
    return np.concatenate(out, axis=0).astype(np.int32) if out else np.zeros((0, 2), np.int32)


def plan_overlap_calls(pairs: np.ndarray, anchor_bytes: np.ndarray, candidate_bytes: np.ndarray, bound: int):
    """The calls of one batch: runs [begin, end) of the candidate-major ``pairs`` such that the bit planes of a run's candidates
    and of the anchors they meet stay within ``bound`` bytes (a run of a single candidate may exceed it: the library decides).
    Candidates are taken in order and never split."""
    k = len(pairs)
    if int(anchor_bytes[np.unique(pairs[:, 1])].sum() + candidate_bytes[np.unique(pairs[:, 0])].sum()) <= bound:
        return [(0, k)]
    starts = np.flatnonzero(np.concatenate([[True], pairs[1:, 0] != pairs[:-1, 0]]))
    ends = np.concatenate([starts[1:], [k]])
    calls, begin, anchors, need = [], 0, set(), 0
    for s, e in zip(starts.tolist(), ends.tolist()):
        met = set(pairs[s:e, 1].tolist())
        own = int(candidate_bytes[pairs[s, 0]])
        more = own + sum(int(anchor_bytes[a]) for a in met - anchors)
        if need and need + more > bound:
            calls.append((begin, s))
            begin, anchors, need = s, set(), 0
            more = own + sum(int(anchor_bytes[a]) for a in met)
        anchors |= met
        need += more
    calls.append((begin, k))
    return calls


def intersected_polygon_ratios(anchor_polygons: Sequence[Polygon], candidate_polygons: Sequence[Polygon],
                               use_candidate_as_base: bool = True, max_scratch_bytes: Optional[int] = None):
    """The batch form of ``PageTextRegionStep.strtree_query_intersected_polygons``: every (candidate, anchor) pair whose
    envelopes meet, with the integer areas and the ratio of ``calculate_boxed_masks_intersected_ratio(anchor.mask,
    candidate.mask, use_candidate_as_base)`` -> (``pairs`` int32 (k, 2) as (candidate, anchor), candidate-major with anchors
    ascending, ``intersected_area`` int64 (k,), ``base_area`` int64 (k,), ``ratio`` float64 (k,)).

    The envelope pairs and the self-relative point tables are built on the host with numpy; the device rasterises every
    polygon that is in a pair once and counts (three launches, one copy-out, one ``Context.sync``; zero pairs: no device call);
    the ratios are ``int64 / int64`` on the host, the correctly rounded float64 of the reference's division.  The bit planes of
    one call are bounded by ``max_scratch_bytes`` (default: VKX_POLY_OVERLAP_MAX_SCRATCH, 1 GiB): a batch that needs more is
    split by candidates into several calls, each rasterising the anchors its candidates meet, still with one synchronisation;
    the result does not depend on the split.  A single candidate whose planes and anchors exceed the bound is refused by the
    library."""
    anchor_polygons, candidate_polygons = list(anchor_polygons), list(candidate_polygons)
    n_anchors = len(anchor_polygons)
    records, points, envelopes = polygon_overlap_tables(anchor_polygons + candidate_polygons)
    pairs = envelope_pairs(envelopes[:n_anchors], envelopes[n_anchors:])
    k = len(pairs)
    intersected_area, base_area = np.zeros(k, np.int64), np.zeros(k, np.int64)
    if k == 0:
        return pairs, intersected_area, base_area, np.zeros(0, np.float64)
    bound = _native.POLY_OVERLAP_MAX_SCRATCH if max_scratch_bytes is None else int(max_scratch_bytes)
    plane_bytes = _native.poly_overlap_plane_bytes(records)
    ctx = _native.default_ctx()
    # the calls: runs of candidates (pairs are candidate-major) whose planes, with those of the anchors they meet, fit the bound
    calls = plan_overlap_calls(pairs, plane_bytes[:n_anchors], plane_bytes[n_anchors:], bound)
    area = np.zeros(len(records), np.int64)
    pending = []
    for s, e in calls:
        part = pairs[s:e].astype(np.int64)
        part[:, 0] += n_anchors
        used, local = np.unique(part, return_inverse=True)
        counts_dev = _native.poly_overlap_counts(records[used], points, local.reshape(-1, 2).astype(np.int32), ctx=ctx)
        counts = ctx.pinned_empty((len(used) + e - s,), np.int32)
        ctx.copy_out(counts_dev.ptr, counts)
        pending.append((s, e, used, counts, counts_dev))
    ctx.sync()
    for s, e, used, counts, _ in pending:
        area[used] = counts[:len(used)]
        intersected_area[s:e] = counts[len(used):]
    if use_candidate_as_base:
        base_area[:] = area[n_anchors + pairs[:, 0]]
    else:
        base_area[:] = area[pairs[:, 1]] + area[n_anchors + pairs[:, 0]] - intersected_area
    if (base_area == 0).any():
        raise ZeroDivisionError('division by zero')
    return pairs, intersected_area, base_area, intersected_area / base_area


# ---- candidate polygons ----------------------------------------------------------------------------------------------
class PageTextRegionStep:
    """What of the reference's step class is pixel work on masks (:868-925, :1115-1216); its host geometry (pyclipper, the
    KD-tree, the minimum-area rectangle) stays outside.  The STR-tree is not needed: the step only asks it which envelopes
    meet (``envelope_pairs``)."""

    @classmethod
    def strtree_query_intersected_polygons(cls, strtree, anchor_polygons: Sequence[Polygon], candidate_polygon: Polygon):
        """The reference's generator (:899-925) of (anchor_idx, anchor_polygon, anchor_mask, candidate_mask,
        intersected_ratio), anchors ascending.  ``strtree`` may be ``None`` and is not consulted: what
        ``sorted(strtree.query(candidate))`` answers is computed from the envelopes of ``anchor_polygons``.  The ratios of all
        answers come from one ``intersected_polygon_ratios`` call; the masks are ``Polygon.mask``."""
        pairs, _, _, ratios = intersected_polygon_ratios(anchor_polygons, [candidate_polygon], use_candidate_as_base=True)
        if len(pairs) == 0:
            return
        candidate_mask = candidate_polygon.mask
        for anchor_idx, intersected_ratio in zip(pairs[:, 1].tolist(), ratios.tolist()):
            anchor_polygon = anchor_polygons[anchor_idx]
            yield anchor_idx, anchor_polygon, anchor_polygon.mask, candidate_mask, intersected_ratio

    @classmethod
    def bind_char_polygons(cls, precise_text_region_polygons: Sequence[Polygon], char_polygons: Sequence[Polygon],
                           max_scratch_bytes: Optional[int] = None):
        """The binding of :1176-1205 for all chars at once -> int32 (len(char_polygons),): the index of the precise text
        region that covers most of the char's mask (the first of equal ratios; a ratio of 0.0 does not bind), -1 for none."""
        bound = np.full(len(char_polygons), -1, np.int32)
        pairs, _, _, ratios = intersected_polygon_ratios(precise_text_region_polygons, char_polygons, use_candidate_as_base=True,
                                                         max_scratch_bytes=max_scratch_bytes)
        if len(pairs) == 0:
            return bound
        # per char (a run of the candidate-major pairs): the first anchor whose ratio is strictly above every earlier one
        # and above 0, i.e. the first position of the run's maximum where that is positive
        starts = np.flatnonzero(np.concatenate([[True], pairs[1:, 0] != pairs[:-1, 0]]))
        lengths = np.diff(np.concatenate([starts, [len(pairs)]]))
        best = np.repeat(np.maximum.reduceat(ratios, starts), lengths)
        position = np.where((ratios == best) & (ratios > 0), np.arange(len(pairs)), len(pairs))
        first = np.minimum.reduceat(position, starts)
        found = first < len(pairs)
        bound[pairs[starts[found], 0]] = pairs[first[found], 1]
        return bound

    @classmethod
    def build_page_text_region_infos(cls, precise_text_region_polygons: Sequence[Polygon], char_polygons: Sequence[Polygon],
                                     max_scratch_bytes: Optional[int] = None):
        """:1160-1216: the precise text regions that received at least one char, in region order, each with its chars in char
        order; a char that no region binds logs the reference's warning and is dropped."""
        bound = cls.bind_char_polygons(precise_text_region_polygons, char_polygons, max_scratch_bytes=max_scratch_bytes)
        ptrp_idx_to_char_polygons = {}
        for char_polygon, ptrp_idx in zip(char_polygons, bound.tolist()):
            if ptrp_idx >= 0:
                ptrp_idx_to_char_polygons.setdefault(ptrp_idx, []).append(char_polygon)
            else:
                logger.warning(f'Cannot assign a text region for char_polygon={char_polygon}')
        return [PageTextRegionInfo(precise_text_region_polygon=precise_text_region_polygon,
                                   char_polygons=ptrp_idx_to_char_polygons[ptrp_idx])
                for ptrp_idx, precise_text_region_polygon in enumerate(precise_text_region_polygons)
                if ptrp_idx in ptrp_idx_to_char_polygons]

    @classmethod
    def find_precise_text_region_candidate_polygons(cls, page_shape: Tuple[int, int],
                                                    disconnected_text_region_polygons: Sequence[Polygon],
                                                    page_resized_text_line_mask: Mask):
        """:1115-1149: the precise polygons of the resized text-line mask, resized back to ``page_shape``, each cut by every
        disconnected text region whose envelope it meets (precise polygons in contour order, regions ascending) -> the flat
        list of candidate polygons.  Composed of ``Mask.to_disconnected_polygons``, ``to_conducted_resized_polygon``,
        ``envelope_pairs`` and ``generate_precise_text_region_candidate_polygons_of_pairs``."""
        page_height, page_width = (int(v) for v in page_shape)
        disconnected_text_region_polygons = list(disconnected_text_region_polygons)
        precise_polygons = [
            resized_precise_polygon.to_conducted_resized_polygon(page_resized_text_line_mask, resized_height=page_height,
                                                                 resized_width=page_width)
            for resized_precise_polygon in page_resized_text_line_mask.to_disconnected_polygons()]
        n_regions = len(disconnected_text_region_polygons)
        _, _, envelopes = polygon_overlap_tables(disconnected_text_region_polygons + precise_polygons)
        pairs = envelope_pairs(envelopes[:n_regions], envelopes[n_regions:])
        if len(pairs) == 0:
            return []
        candidates = cls.generate_precise_text_region_candidate_polygons_of_pairs(
            [(precise_polygons[c].mask, disconnected_text_region_polygons[a].mask) for c, a in pairs.tolist()])
        return [polygon for polygons in candidates for polygon in polygons]

    @classmethod
    def _intersected_mask(cls, precise_mask: Mask, disconnected_text_region_mask: Mask):
        assert precise_mask.box and disconnected_text_region_mask.box
        intersected_box = Box(up=max(precise_mask.box.up, disconnected_text_region_mask.box.up),
                              down=min(precise_mask.box.down, disconnected_text_region_mask.box.down),
                              left=max(precise_mask.box.left, disconnected_text_region_mask.box.left),
                              right=min(precise_mask.box.right, disconnected_text_region_mask.box.right))
        assert intersected_box.up <= intersected_box.down
        assert intersected_box.left <= intersected_box.right
        # the reference's `a.mat & b.mat` of two 0 / 1 planes: active where both are (one vkx_set_mask call, each mask read
        # through its window over the box)
        from vkit_amd.element.type import ElementSetOperationMode
        return Mask.from_masks(intersected_box, [disconnected_text_region_mask, precise_mask], ElementSetOperationMode.INTERSECT)

    @classmethod
    def generate_precise_text_region_candidate_polygons(cls, precise_mask: Mask, disconnected_text_region_mask: Mask):
        # 1. Could extract more than one polygons.  2. Some polygons are in border and should be removed later.
        return cls._intersected_mask(precise_mask, disconnected_text_region_mask).to_disconnected_polygons()

    @classmethod
    def generate_precise_text_region_candidate_polygons_of_pairs(cls, pairs):
        """``generate_precise_text_region_candidate_polygons`` of every (precise_mask, disconnected_text_region_mask) pair of
        ``pairs`` -> a list of lists; the contours of all pairs come from ONE contour call."""
        from vkit_amd.element.mask import masks_to_disconnected_polygons
        return masks_to_disconnected_polygons([cls._intersected_mask(precise, region) for precise, region in pairs])


# ---- stacking ------------------------------------------------------------------------------------------------------
def build_background_image_for_stacking(height: int, width: int):
    """Channel k of pixel (y, x) is 255 exactly when k == (y + x) % 3 (the reference's three row patterns, :732-745)."""
    if _native.resident_mode():
        image, _ = _native.region_stack(np.zeros(0, _native.REGION_STACK_ITEM_DTYPE), (height, width))
        return Image(mat=image)
    phase = (np.arange(height)[:, None] + np.arange(width)[None, :]) % 3
    return Image(mat=((phase[:, :, None] == np.arange(3)) * 255).astype(np.uint8))


class ColumnPacker:
    """The packer ``stack_flattened_text_regions`` falls back to without rectpack: rectangles one below the other in the order
    they were added, all at x = 0.  The reference's only bin is (widest rectangle) x (sum of the heights), so the column
    always fits.  The calls are the four of rectpack's packer that the reference uses."""

    def __init__(self):
        self.rects, self.bins, self.placed = [], [], []

    def add_rect(self, width, height, rid=None):
        self.rects.append((width, height, rid))

    def add_bin(self, width, height):
        self.bins.append((width, height))

    def pack(self):
        y = 0
        self.placed = []
        for width, height, rid in self.rects:
            self.placed.append((0, 0, y, width, height, rid))
            y += height

    def rect_list(self):
        return list(self.placed)


def default_rect_packer_factory():
    try:
        from rectpack import newPacker
    except ImportError:
        return ColumnPacker()
    return newPacker(rotation=False)


def stack_flattened_text_regions(page_pad: int, flattened_text_regions_pad: int,
                                 flattened_text_regions: Sequence[FlattenedTextRegion], rect_packer_factory=None):
    """The reference's function (:748-856) with its packer as an argument: any object with ``add_rect``, ``add_bin``, ``pack``
    and ``rect_list``.  One launch writes the striped page, the regions under their masks and the active mask."""
    regions = list(flattened_text_regions)
    page_double_pad = 2 * page_pad
    double_pad = 2 * flattened_text_regions_pad
    rect_packer = (rect_packer_factory or default_rect_packer_factory)()

    bin_width = bin_height = 0
    for ftr_idx, region in enumerate(regions):
        rect_packer.add_rect(width=region.width + double_pad, height=region.height + double_pad, rid=ftr_idx)
        bin_width = max(bin_width, region.width)
        bin_height += region.height
    rect_packer.add_bin(width=bin_width + double_pad, height=bin_height + double_pad)
    rect_packer.pack()

    padded_boxes: List[Optional[Box]] = [None] * len(regions)
    for bin_idx, x, y, width, height, ftr_idx in rect_packer.rect_list():
        assert bin_idx == 0
        padded_boxes[ftr_idx] = Box(up=y, down=y + height - 1, left=x, right=x + width - 1)
    assert all(box is not None for box in padded_boxes)

    page_height = max(box.down for box in padded_boxes) + 1 + page_double_pad
    page_width = max(box.right for box in padded_boxes) + 1 + page_double_pad

    src = _region_sources(regions)
    items = np.zeros(len(regions), _native.REGION_STACK_ITEM_DTYPE)
    text_region_boxes: List[Box] = []
    char_polygons: List[Polygon] = []
    char_polygon_text_region_box_indices: List[int] = []
    for k, (padded_box, region) in enumerate(zip(padded_boxes, regions)):
        assert region.height + double_pad == padded_box.height
        assert region.width + double_pad == padded_box.width
        assert region.flattened_image.shape == region.flattened_mask.shape
        up = padded_box.up + flattened_text_regions_pad + page_pad
        left = padded_box.left + flattened_text_regions_pad + page_pad
        text_region_boxes.append(Box(up=up, down=up + region.height - 1, left=left, right=left + region.width - 1))
        item = items[k]
        item['image'], item['mask'] = src.ptr[2 * k], src.ptr[2 * k + 1]
        item['h'], item['w'], item['up'], item['left'] = region.height, region.width, up, left
        if region.flattened_char_polygons:
            for char_polygon in region.flattened_char_polygons:
                char_polygons.append(char_polygon.to_shifted_polygon(offset_y=up, offset_x=left))
                char_polygon_text_region_box_indices.append(k)
    image, active_mask = _native.region_stack(items, (page_height, page_width), ctx=src.ctx)
    if not src.resident:
        image, active_mask = np.array(image.host()), np.array(active_mask.host())
    return Image(mat=image), Mask(mat=active_mask), text_region_boxes, char_polygons, char_polygon_text_region_box_indices
