#!/usr/bin/env python3
"""Regenerates tests/golden/text_region_label.npz by running THE REFERENCE's own PageTextRegionLabelStep
(vkit/pipeline/text_detection/page_text_region_label.py) on small synthetic pages.

    python tests/golden/make_text_region_label_golden.py

The missing third-party modules are stubbed exactly as make_golden.py stubs them (it is imported for that).  Three cv2 calls
are oracle-patched (cv.getPerspectiveTransform, cv.warpPerspective, cv.fillPoly, as in make_char_heatmap_golden.py), and
Polygon.get_center_point takes the project's restatement of the shapely centroid (vkit_amd.element.polygon.polygon_centroids).
sklearn's KDTree is the real one.  Everything else -- the sort, the fills, the draws, affine_points, the label objects, the
box mask and the exceptions -- is the reference's code running for real.

Stored per case, in one JSON ``index`` row: the config, the page shape, the seed, the generator state after the run, the
warning count, the exception type of the raising cases, and where the inputs (quads float64, active mask) and the results
(the four planes, every label, the label-class measures, shifted and downsampled copies of a few labels) sit in a few flat
arrays.  Data only.
"""
import json
import logging
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402,F401  (stubs cv2 & co., puts the reference and this repository on sys.path)

import numpy as np  # noqa: E402
from numpy.random import default_rng  # noqa: E402

import cv2 as cv_stub  # noqa: E402  (the MagicMock)
import oracle as O  # noqa: E402
from vkit.element import Image, Mask, Point, PointList, Polygon  # noqa: E402
from vkit.pipeline.text_detection.page_text_region import PageTextRegionStepOutput  # noqa: E402
from vkit.pipeline.text_detection import page_text_region_label as L  # noqa: E402
from vkit.engine.char_heatmap.type import CharHeatmapEngineRunConfig  # noqa: E402
from vkit_amd.element.polygon import polygon_centroids  # noqa: E402

OUT = os.path.join(HERE, 'text_region_label.npz')


def _fill_poly(img, pts_list, color):
    assert color == 1 and len(pts_list) == 1
    m = O.fill_poly(img.shape, pts_list[0])
    img[m > 0] = 1
    return img


cv_stub.getPerspectiveTransform = lambda a, b, *rest: O.get_perspective_transform(a, b)
cv_stub.warpPerspective = lambda src, M, dsize, *rest, **kw: O.warp_perspective(src, M, (int(dsize[0]), int(dsize[1])))
cv_stub.fillPoly = _fill_poly


def _center(self):
    xy = np.asarray(self.to_smooth_xy_pairs(), np.float64)
    x, y = polygon_centroids(xy[None])[0].tolist()
    return Point.create(y=y, x=x)


Polygon.get_center_point = _center


class _Count(logging.Handler):
    def __init__(self):
        super().__init__()
        self.n = 0

    def emit(self, record):
        self.n += 1


COUNT = _Count()
L.logger.addHandler(COUNT)
L.logger.propagate = False


def quad(cx, cy, sw, sh, kind, rng):
    """one char quad (4, 2) float64 (x, y) centred at (cx, cy), sw x sh: 'axis', 'rot', 'shear' or 'persp'"""
    q = np.array([(-1, -1), (1, -1), (1, 1), (-1, 1)], np.float64) * (sw / 2, sh / 2)
    if kind in ('rot', 'shear', 'persp'):
        a = rng.uniform(-0.6, 0.6)
        q = q @ np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]]).T
    if kind in ('shear', 'persp'):
        q = q @ np.array([[1, rng.uniform(-0.4, 0.4)], [rng.uniform(-0.3, 0.3), 1]]).T
    if kind == 'persp':
        q = q + rng.uniform(-0.15, 0.15, (4, 2)) * max(sw, sh)
    return np.round(q + (cx, cy), 3)


def scatter(rng, shape, n, size, kinds):
    h, w = shape
    out = []
    for k in range(n):
        s = rng.uniform(*size)
        out.append(quad(rng.uniform(s, w - s), rng.uniform(s, h - s), s * rng.uniform(0.7, 1.0), s, kinds[k % len(kinds)], rng))
    return np.asarray(out).reshape(-1, 4, 2)


def grid(shape, rows, cols, size, origin=(2, 2), pitch=None):
    """a regular grid of axis-aligned chars on integer positions: equidistant centres, ties in the nearest-centre test"""
    pitch = pitch or size
    out = []
    for r in range(rows):
        for c in range(cols):
            x0, y0 = origin[0] + c * pitch, origin[1] + r * pitch
            out.append([(x0, y0), (x0 + size, y0), (x0 + size, y0 + size), (x0, y0 + size)])
    return np.asarray(out, np.float64)


def active_mask(shape, rng, kind):
    m = np.ones(shape, np.uint8)
    if kind == 'holes':
        h, w = shape
        for _ in range(3):
            y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
            m[y:y + int(rng.integers(3, h // 2 + 4)), x:x + int(rng.integers(3, w // 2 + 4))] = 0
    return m


def polygons_of(qs):
    return [Polygon.create(points=PointList(Point.create(y=float(y), x=float(x)) for x, y in q)) for q in qs]


def main():
    packed, index = {}, []

    def put(key, array):
        array = np.ascontiguousarray(array)
        flat = packed.setdefault(key, [])
        at = sum(a.size for a in flat)
        flat.append(array.reshape(-1))
        return [at, list(array.shape), str(array.dtype)]

    def case(name, shape, qs, num=1, factor=3, seed=0, active='holes', shift=(3, -2), factor_down=2):
        qs = [np.asarray(q, np.float64) for q in qs]
        rng = default_rng(seed)
        act = active_mask(shape, default_rng(seed + 1000), active)
        row = dict(name=name, shape=list(shape), num=num, factor=factor, seed=seed, active=put('u8', act),
                   quads=put('f64', np.asarray(qs, np.float64).reshape(-1, np.asarray(qs[0]).shape[0] if qs else 4, 2)),
                   shift=list(shift), factor_down=factor_down)
        step = L.PageTextRegionLabelStep(L.PageTextRegionLabelStepConfig(
            num_deviate_char_regression_labels=num, num_deviate_char_regression_labels_candiates_factor=factor))
        # the executor structures a mapping with cattrs (stubbed here): hand it the run config itself
        engine = step.char_heatmap_default_engine_executor.engine
        step.char_heatmap_default_engine_executor.run = lambda config, rng=None: engine.run(CharHeatmapEngineRunConfig(**config))
        polygons = polygons_of(qs)
        src = PageTextRegionStepOutput(page_image=Image(mat=np.zeros(shape + (3,), np.uint8)), page_active_mask=Mask(mat=act),
                                       page_char_polygons=polygons, page_text_region_polygons=polygons,
                                       page_char_polygon_text_region_polygon_indices=list(range(len(polygons))),
                                       shape_before_rotate=shape, rotate_angle=0, debug=None)
        COUNT.n = 0
        try:
            out = step.run(L.PageTextRegionLabelStepInput(page_text_region_step_output=src), rng)
        except Exception as e:      # noqa: BLE001  (the reference's own exception is the expectation)
            row['raises'] = type(e).__name__
        else:
            row['char_mask'] = put('u8', out.page_char_mask.mat)
            row['height'] = put('f32', out.page_char_height_score_map.mat)
            row['gaussian'] = put('f32', out.page_char_gaussian_score_map.mat)
            row['box_mask'] = put('u8', out.page_char_bounding_box_mask.mat)
            labels = out.page_char_regression_labels
            row['label_char'] = put('i64', np.array([lb.char_idx for lb in labels], np.int64))
            row['label_tag'] = put('i64', np.array([lb.tag == L.PageCharRegressionLabelTag.DEVIATE for lb in labels], np.int64))
            row['label_smooth'] = put('f64', np.array([(lb.label_point_smooth_y, lb.label_point_smooth_x) for lb in labels],
                                                      np.float64).reshape(-1, 2))
            row['label_int'] = put('i64', np.array([(lb.downsampled_label_point_y, lb.downsampled_label_point_x)
                                                    for lb in labels], np.int64).reshape(-1, 2))
            row['label_valid'] = put('i64', np.array([lb.valid for lb in labels], np.int64))
            row['label_orientation'] = put('i64', np.array([lb.bounding_orientation_idx for lb in labels], np.int64))
            row['label_offsets'] = put('f64', np.array([lb.generate_up_left_offsets() for lb in labels],
                                                       np.float64).reshape(-1, 2))
            row['label_angles'] = put('f64', np.array([lb.generate_clockwise_angle_distribution() for lb in labels],
                                                      np.float64).reshape(-1, 4))
            row['label_distances'] = put('f64', np.array([lb.generate_clockwise_distances() for lb in labels],
                                                         np.float64).reshape(-1, 4))
            few = [lb for lb in labels if lb.valid][:3]
            shifted = [lb.to_shifted_page_char_regression_label(offset_y=shift[0], offset_x=shift[1]) for lb in few]
            down = [lb.to_downsampled_page_char_regression_label(factor_down) for lb in few]
            row['shifted'] = put('f64', np.array([
                (s.label_point_smooth_y, s.label_point_smooth_x, s.downsampled_label_point_y, s.downsampled_label_point_x,
                 s.up_left.smooth_y, s.up_left.smooth_x, s.down_right.smooth_y, s.down_right.smooth_x,
                 s.bounding_smooth_up, s.bounding_smooth_left, float(s.valid)) for s in shifted], np.float64).reshape(-1, 11))
            row['downsampled'] = put('f64', np.array([
                (d.downsampled_label_point_y, d.downsampled_label_point_x, float(d.is_downsampled), d.downsample_labeling_factor,
                 d.label_point_smooth_y, d.label_point_smooth_x) for d in down], np.float64).reshape(-1, 6))
        row['warnings'] = COUNT.n
        state = rng.bit_generator.state['state']
        row['rng_state'] = [str(state['state']), str(state['inc'])]
        index.append(row)

    rng = default_rng(20261016)
    shape = (48, 64)
    for kind in ('axis', 'rot', 'shear', 'persp'):
        case(f'scatter-{kind}', shape, scatter(rng, shape, 5, (8, 16), [kind]), seed=len(index))
    case('mixed-num0', shape, scatter(rng, shape, 6, (8, 16), ['axis', 'rot', 'persp']), num=0, seed=len(index))
    case('mixed-num3', shape, scatter(rng, shape, 6, (8, 16), ['axis', 'rot', 'persp']), num=3, seed=len(index))
    case('mixed-num3-factor2', shape, scatter(rng, shape, 6, (8, 16), ['shear', 'persp']), num=3, factor=2, seed=len(index))
    case('mixed-num1-factor1', shape, scatter(rng, shape, 6, (8, 16), ['rot']), num=1, factor=1, seed=len(index))
    case('overlapping', shape, scatter(rng, (30, 40), 8, (8, 12), ['axis', 'rot', 'persp']), num=2, seed=len(index))
    case('all-active', shape, scatter(rng, shape, 6, (8, 16), ['rot']), active='all', seed=len(index))
    case('small-chars', shape, scatter(rng, shape, 10, (3, 6), ['axis', 'rot']), num=2, seed=len(index))
    case('grid-6x10', (56, 88), grid((56, 88), 6, 10, 8), num=3, seed=len(index))
    case('grid-7x9-touching', (80, 96), grid((80, 96), 7, 9, 10, pitch=10), num=2, seed=len(index))
    case('grid-5x9-overlap', (60, 90), grid((60, 90), 5, 9, 10, pitch=9), num=1, seed=len(index))
    case('grid-8x8-num0', (72, 72), grid((72, 72), 8, 8, 8), num=0, seed=len(index))
    for seed in range(3):
        case(f'dense-{seed}', (64, 80), scatter(rng, (64, 80), 40, (6, 14), ['axis', 'rot', 'shear', 'persp']), num=2,
             seed=100 + seed)
    # the raising cases
    case('no-chars', shape, [], seed=len(index))
    case('three-points', shape, [np.array([(5, 5), (15, 5), (10, 12)], np.float64)], seed=len(index))
    case('small-box-height', shape, [quad(20, 20, 10, 10, 'axis', rng), np.array([(30, 30), (40, 30), (40, 31), (30, 31.2)])],
         seed=len(index))
    case('small-box-width', shape, [quad(20, 20, 10, 10, 'axis', rng), np.array([(30, 30), (31, 30), (31.2, 40), (30, 40)])],
         seed=len(index))
    case('small-box-num0', shape, [np.array([(30, 30), (31, 30), (31.2, 40), (30, 40)])], num=0, seed=len(index))
    dart = np.array([(10, 10), (40, 10), (16, 16), (10, 40)], np.float64)
    case('concave-candidate-outside', (48, 48), [quad(30, 36, 8, 8, 'axis', rng), dart], num=3, seed=len(index))
    case('box-past-the-page', shape, [quad(20, 20, 10, 10, 'rot', rng),
                                      np.array([(30, -0.3), (40, -0.2), (40, 9), (30, 9)], np.float64)], seed=len(index))
    case('page-shaped-box', (20, 30), [np.array([(-0.4, -0.3), (27.7, -0.2), (27.6, 17.6), (-0.3, 17.5)], np.float64)],
         seed=len(index))
    case('box-at-the-edge', (20, 30), [np.array([(20, 10), (29.4, 10), (29.4, 19.4), (20, 19.4)], np.float64)],
         seed=len(index))

    out = {k: np.concatenate(v) for k, v in packed.items()}
    out['index'] = np.array(json.dumps(index))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes,', len(index), 'cases,', sum('raises' in r for r in index), 'raising:',
          sorted({(r['name'], r['raises']) for r in index if 'raises' in r}))
    print('warnings', {r['name']: r['warnings'] for r in index if r['warnings']})


if __name__ == '__main__':
    main()
