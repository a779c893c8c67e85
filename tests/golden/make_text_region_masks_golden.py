#!/usr/bin/env python3
"""Regenerates tests/golden/text_region_masks.npz by running THE REFERENCE's own
TextRegionFlattener.get_bounding_extended_text_region_masks (vkit/pipeline/text_detection/page_text_region.py:477-558) and
Polygon.to_bounding_rectangular_polygon(shape, angle) (vkit/element/polygon.py:359-434) on small synthetic pages:

    python tests/golden/make_text_region_masks_golden.py

The missing third-party modules are stubbed as make_golden.py stubs them (it is imported for that); cv.fillPoly is the
oracle's, as in make_text_region_flatten_golden.py.

Cases (tests/text_region_masks_restate.py: make_case): pages of 96 x 128 and 61 x 203; 1, 3 and 70 regions a page, three seeds
each, every page once with typical_indices empty (no rectangle is patched) and once with every second region typical (the
others get the rectangle of their main angle: 0, 1, 45, 89, 90, 91, 135, 179).  Regions: boxes of 1 x 1, 1 x N and N x 1 (a
single point, a two-point and a collinear polygon), one on the top and left page borders and one on the bottom and right
borders, D == O, rectangles that do not contain D, a region nested in another, a neighbour whose rectangle covers another
region's polygon, a comb of 48 vertices and one of 68.  Then the rectangle of every angle for a few polygons, called directly.
Stored: point tables, typical indices, angles, the patched rectangles and every output mask with its box.  Data only, never
reference source text.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402,F401  (stubs cv2 & co., puts the reference and this repository on sys.path)

sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

import cv2 as cv_stub  # noqa: E402  (the MagicMock)
import text_region_masks_restate as R  # noqa: E402
from make_text_region_flatten_golden import _fill_poly  # noqa: E402
from vkit.element import Polygon  # noqa: E402
from vkit.pipeline.text_detection import page_text_region as TR  # noqa: E402

OUT = os.path.join(HERE, 'text_region_masks.npz')
SEEDS = (0, 1, 2)


def polygon_of(points):
    return Polygon.from_xy_pairs([(int(x), int(y)) for x, y in points])


def points_of(polygon):
    return np.array([(p.x, p.y) for p in polygon.points], np.int32)


def main():
    cv_stub.fillPoly = _fill_poly
    packed, runs, rectangles = {}, [], []

    def put(array):
        array = np.ascontiguousarray(array)
        flat = packed.setdefault(str(array.dtype), [])
        at = sum(a.size for a in flat)
        flat.append(array.reshape(-1))
        return [at, list(array.shape), str(array.dtype)]

    for shape in R.PAGES:
        for n in R.COUNTS:
            for seed in SEEDS:
                regions, angles = R.make_case(R.case_rng(shape, n, seed), shape, n)
                originals = [polygon_of(o) for o, _, _ in regions]
                dilated = [polygon_of(d) for _, d, _ in regions]
                given = [polygon_of(r) for _, _, r in regions]
                for typical in ([], list(range(0, n, 2))):
                    masks = TR.TextRegionFlattener.get_bounding_extended_text_region_masks(
                        shape, originals, dilated, given, typical, angles)
                    patched = [points_of(d.to_bounding_rectangular_polygon(shape=shape, angle=angles[k]))
                               if typical and k not in typical else None for k, d in enumerate(dilated)]
                    assert len(masks) == n
                    runs.append(dict(
                        shape=list(shape), n=n, seed=seed, typical=typical, angles=angles,
                        regions=[dict(original=put(o), dilated=put(d), rectangle=put(r),
                                      patched=None if patched[k] is None else put(patched[k]))
                                 for k, (o, d, r) in enumerate(regions)],
                        masks=[dict(mat=put(m.mat), box=[m.box.up, m.box.down, m.box.left, m.box.right]) for m in masks]))
    # the rectangle of every angle, called directly (float angles and angles outside [0, 180) too)
    rng = np.random.default_rng(77)
    for shape in R.PAGES:
        regions, _ = R.make_case(rng, shape, 14)
        for k, (_, d, _) in enumerate(regions):
            for angle in R.ANGLES + (180, 270.5, -30, 12.25):
                rectangles.append(dict(shape=list(shape), points=put(d), angle=angle,
                                       rectangle=put(points_of(polygon_of(d).to_bounding_rectangular_polygon(shape=shape, angle=angle)))))
    # (the two errors of the intersection are raised by the reference on the arguments the test uses)
    for args, message in (((np.zeros(2), np.pi / 2, np.ones(2), np.pi / 2), 'Lines are vertical.'),
                          ((np.zeros(2), 0.3, np.array([0.0, 1.0]), 0.3), 'Lines not intersected.')):
        try:
            Polygon.calculate_lines_intersection_point(*args)
        except RuntimeError as error:
            assert str(error) == message
        else:
            raise AssertionError(message)
    out = {k: np.concatenate(v) for k, v in packed.items()}
    out['index'] = np.array(json.dumps(dict(runs=runs, rectangles=rectangles)))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes', len(runs), 'runs', len(rectangles), 'rectangles')


if __name__ == '__main__':
    main()
