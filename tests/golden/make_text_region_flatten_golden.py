#!/usr/bin/env python3
"""Regenerates tests/golden/text_region_flatten.npz by running THE REFERENCE's own pixel half of PageTextRegionStep
(vkit/pipeline/text_detection/page_text_region.py) on small synthetic pages, three seeds a case:

    python tests/golden/make_text_region_flatten_golden.py

TextRegionFlattener.build_flattened_text_regions, FlattenedTextRegion.to_resized_flattened_text_region,
.to_post_rotated_flattened_text_region and stack_flattened_text_regions run for real.  The missing third-party modules are
stubbed as make_golden.py stubs them (it is imported for that); cv.warpAffine, cv.resize and cv.fillPoly are the oracle's; the
cattrs stub gets its ``structure`` (``cls(**mapping)``: the region methods hand rotate.distort a mapping); the stubbed
RectPacker is replaced by the stand-in below, which shelves the rectangles in rows in descending order of height, so that the
placement is not the order of the regions.

Cases: pages of 96 x 128 and 61 x 203; 1, 3 and 70 regions a page; region boxes 1 x N, N x 1 and 5 .. 40 px a side, one
touching each page border, one whose mask is a single pixel, one whose mask is full; flattening angles 1, 45, 89, 90, 91, 135,
180, 269, 270, 359; resizes up, down and to a height of 1; post-rotations by 0, 90, 180 and 270 degrees.  A region whose
rotated mask comes out empty (the reference raises) is turned by 90 degrees instead.  Pages and masks are blocky so that the
file stays small.  Stored: inputs, every region's planes, boxes and shapes after each operation, the packer's placements, the
stacked image and mask, and the char polygons.  Data only, never reference source text.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402,F401  (stubs cv2 & co., puts the reference and this repository on sys.path)

import numpy as np  # noqa: E402
from numpy.random import default_rng  # noqa: E402

import cv2 as cv_stub  # noqa: E402  (the MagicMock)
import oracle as O  # noqa: E402
from make_cropping_golden import blocky  # noqa: E402
from vkit.element import Box, Image, Mask, Polygon  # noqa: E402
from vkit.pipeline.text_detection import page_text_region as TR  # noqa: E402
from vkit.utility import opt as ref_opt  # noqa: E402

OUT = os.path.join(HERE, 'text_region_flatten.npz')
ANGLES = (1, 45, 89, 90, 91, 135, 180, 269, 270, 359)
PAGES = ((96, 128), (61, 203))
COUNTS = (1, 3, 70)
SEEDS = (0, 1, 2)


class ShelfPacker:
    """rectpack's four calls: rectangles sorted by descending height (ties by rid) onto shelves of the bin's width"""

    def __init__(self, rotation=False):
        assert rotation is False
        self.rects, self.bin, self.placed = [], None, []

    def add_rect(self, width, height, rid=None):
        self.rects.append((width, height, rid))

    def add_bin(self, width, height):
        assert self.bin is None
        self.bin = (width, height)

    def pack(self):
        x = y = shelf = 0
        for width, height, rid in sorted(self.rects, key=lambda r: (-r[1], r[2])):
            if x and x + width > self.bin[0]:
                x, y, shelf = 0, y + shelf, 0
            self.placed.append((0, x, y, width, height, rid))
            x, shelf = x + width, max(shelf, height)

    def rect_list(self):
        return list(self.placed)


def _fill_poly(img, pts_list, color):
    assert len(pts_list) == 1
    m = O.fill_poly(img.shape, pts_list[0])
    img[m > 0] = color


def make_case(rng, shape, n):
    h, w = shape
    page = np.stack([blocky(rng, shape, 8, 0, 16, np.uint8) * np.uint8(17) for _ in range(3)], axis=2)
    special = [(0, 0, 9, 17, 'rand'), (h - 7, 3, 7, 11, 'rand'), (5, 0, 12, 6, 'rand'), (2, w - 9, 8, 9, 'rand'),
               (10, 20, 9, 13, 'pixel'), (20, 30, 6, 21, 'full'), (30, 5, 1, 23, 'full'), (3, 40, 19, 1, 'full')]
    regions = []
    for k in range(n):
        if n > 3 and k < len(special):
            up, left, bh, bw, kind = special[k]
        else:
            bh, bw = int(rng.integers(5, 41)), int(rng.integers(5, 41))
            up, left, kind = int(rng.integers(0, h - bh + 1)), int(rng.integers(0, w - bw + 1)), 'rand'
        if kind == 'full':
            mat = np.ones((bh, bw), np.uint8)
        elif kind == 'pixel':
            mat = np.zeros((bh, bw), np.uint8)
            mat[bh // 2, bw // 2] = 1
        else:
            mat = (blocky(rng, (bh, bw), 3, 0, 5, np.uint8) > 0).astype(np.uint8)
            mat[bh // 2, bw // 2] = 1
        chars = []
        for _ in range(int(rng.integers(0, 3))):
            cy, cx = rng.uniform(up, up + bh), rng.uniform(left, left + bw)
            q = np.array([(-2, -3), (-2, 3), (2, 3), (2, -3)]) + rng.uniform(-0.6, 0.6, (4, 2)) + (cy, cx)
            chars.append(np.round(q, 3))
        regions.append(dict(box=[up, up + bh - 1, left, left + bw - 1], mask=mat, angle=ANGLES[k % len(ANGLES)], chars=chars))
    return page, regions


def polygon_of(q):
    return Polygon.from_np_array(np.ascontiguousarray(q[:, ::-1], dtype=np.float32))


def polygons_xy(polygons):
    if polygons is None:
        return None
    return [np.array([(p.smooth_x, p.smooth_y) for p in polygon.points], np.float64) for polygon in polygons]


def main():
    cv_stub.warpAffine = lambda mat, trans_mat, dsize: O.warp_affine(mat, trans_mat, dsize)
    cv_stub.resize = lambda mat, dsize, interpolation=None: O.resize(mat, (dsize[1], dsize[0]), interpolation)
    cv_stub.fillPoly = _fill_poly
    ref_opt._cattrs.structure = lambda mapping, cls: cls(**mapping)
    TR.RectPacker = ShelfPacker
    packed, runs = {}, []

    def put(array):
        array = np.ascontiguousarray(array)
        flat = packed.setdefault(str(array.dtype), [])
        at = sum(a.size for a in flat)
        flat.append(array.reshape(-1))
        return [at, list(array.shape), str(array.dtype)]

    def put_region(region):
        box = region.rotated_trimmed_box
        xy = polygons_xy(region.flattened_char_polygons)
        return dict(image=put(region.flattened_image.mat), mask=put(region.flattened_mask.mat),
                    shape_before_trim=list(region.shape_before_trim), shape_before_resize=list(region.shape_before_resize),
                    rotated_trimmed_box=[box.up, box.down, box.left, box.right], post_rotate_angle=region.post_rotate_angle,
                    is_typical=bool(region.is_typical), chars=None if xy is None else [put(q) for q in xy])

    for shape in PAGES:
        for n in COUNTS:
            for seed in SEEDS:
                rng = default_rng(1_000_000 + 1000 * n + 10 * shape[0] + seed)
                page, regions = make_case(rng, shape, n)
                image = Image(mat=page)
                masks = [Mask(mat=r['mask']).to_box_attached(Box(up=r['box'][0], down=r['box'][1], left=r['box'][2],
                                                                  right=r['box'][3])) for r in regions]
                grouped = [[polygon_of(q) for q in r['chars']] for r in regions]
                polygons = [None] * n          # passed through untouched
                typical = list(range(0, n, 2))
                for k, r in enumerate(regions):       # an empty rotated mask raises: turn that region by 90 degrees instead
                    try:
                        TR.TextRegionFlattener.build_flattened_text_regions(image, polygons[k:k + 1], masks[k:k + 1], (), [r['angle']], None)
                    except RuntimeError:
                        r['angle'] = 90
                angles = [r['angle'] for r in regions]
                built = TR.TextRegionFlattener.build_flattened_text_regions(image, polygons, masks, typical, angles, grouped)
                row = dict(shape=list(shape), n=n, seed=seed, page=put(page), typical=typical,
                           regions=[dict(box=r['box'], mask=put(r['mask']), angle=r['angle'],
                                         chars=[put(q) for q in r['chars']]) for r in regions],
                           text_region_image0=put(built[0].text_region_image.mat), built=[put_region(r) for r in built])
                # resize: to a height of 1, to a width of 7, up, down; only regions whose image and mask agree go on
                keep = [k for k, r in enumerate(built) if r.flattened_image.shape == r.flattened_mask.shape]
                targets = []
                for k in keep:
                    h, w = built[k].shape
                    # (an aspect that would round the free side to 0 gets both sides)
                    targets.append([(1, None if round(w / h) else 1), (None if round(7 * h / w) else 1, 7), (h + 3, w + 2),
                                    (max(h // 2, 1), max(w // 3, 1))][k % 4])
                resized = [built[k].to_resized_flattened_text_region(*t) for k, t in zip(keep, targets)]
                post = [(0, 90, 180, 270)[i % 4] for i in range(len(keep))]
                rotated = [r if a == 0 else r.to_post_rotated_flattened_text_region(a) for r, a in zip(resized, post)]
                row.update(keep=keep, targets=[list(t) for t in targets], resized=[put_region(r) for r in resized], post=post,
                           rotated=[put_region(r) if a else None for r, a in zip(rotated, post)])   # (angle 0: the resized region itself)
                if rotated:
                    packer = []
                    TR.RectPacker = lambda rotation=False: packer.append(ShelfPacker(rotation)) or packer[-1]
                    stacked = TR.stack_flattened_text_regions(1, 2, rotated)
                    TR.RectPacker = ShelfPacker
                    row['stack'] = dict(page_pad=1, pad=2, placements=[list(p) for p in packer[0].rect_list()],
                                        image=put(stacked[0].mat), mask=put(stacked[1].mat),
                                        boxes=[[b.up, b.down, b.left, b.right] for b in stacked[2]],
                                        chars=[put(q) for q in polygons_xy(stacked[3])], char_box_indices=list(stacked[4]))
                runs.append(row)
    out = {k: np.concatenate(v) for k, v in packed.items()}
    out['background_7x11'] = TR.build_background_image_for_stacking(7, 11).mat
    out['index'] = np.array(json.dumps(dict(runs=runs)))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes', len(runs), 'runs')


if __name__ == '__main__':
    main()
