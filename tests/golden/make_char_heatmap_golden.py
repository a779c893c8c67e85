#!/usr/bin/env python3
"""Regenerates tests/golden/char_heatmap.npz by running THE REFERENCE's own default char-heatmap engine
(vkit/engine/char_heatmap/default.py) on small synthetic pages.

    python tests/golden/make_char_heatmap_golden.py

The missing third-party modules are stubbed exactly as make_golden.py stubs them (it is imported for that).  Three cv2 calls
are oracle-patched: cv.getPerspectiveTransform becomes oracle.get_perspective_transform, cv.warpPerspective
oracle.warp_perspective and cv.fillPoly oracle.fill_poly.  Everything else -- the template, the keep-max / keep-min fills,
Mask.from_polygons, the numpy tail and the exceptions -- is the reference's code running for real.

Stored per case, in one JSON ``index`` row: the config, the page shape, where the quads (float64) and the expected planes
sit in a few flat arrays, and the exception type for the raising cases.  Data only.
"""
import json
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
from vkit.element import Point, PointList, Polygon  # noqa: E402
from vkit.engine.char_heatmap.default import (  # noqa: E402
    CharHeatmapDefaultEngine, CharHeatmapDefaultEngineInitConfig)
from vkit.engine.char_heatmap.type import CharHeatmapEngineRunConfig  # noqa: E402

OUT = os.path.join(HERE, 'char_heatmap.npz')


def _fill_poly(img, pts_list, color):
    assert color == 1 and len(pts_list) == 1
    m = O.fill_poly(img.shape, pts_list[0])
    img[m > 0] = 1
    return img


cv_stub.getPerspectiveTransform = lambda a, b, *rest: O.get_perspective_transform(a, b)
cv_stub.warpPerspective = lambda src, M, dsize, *rest, **kw: O.warp_perspective(src, M, (int(dsize[0]), int(dsize[1])))
cv_stub.fillPoly = _fill_poly

DEBUG_NAMES = ('score_map_max', 'score_map_min', 'char_overlapped_mask', 'char_neutralized_score_map', 'neutralized_mask',
               'neutralized_score_map')


def quad(cx, cy, sw, sh, kind, rng):
    """one char quad (4, 2) float64 (x, y) centred at (cx, cy), sw x sh: 'axis', 'rot', 'shear' or 'persp'"""
    q = np.array([(-1, -1), (1, -1), (1, 1), (-1, 1)], np.float64) * (sw / 2, sh / 2)
    if kind in ('rot', 'shear', 'persp'):
        a = rng.uniform(-0.6, 0.6)
        q = q @ np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]]).T
    if kind in ('shear', 'persp'):
        q = q @ np.array([[1, rng.uniform(-0.4, 0.4)], [rng.uniform(-0.3, 0.3), 1]]).T
    if kind == 'persp':
        q = q + rng.uniform(-0.2, 0.2, (4, 2)) * max(sw, sh)
    return np.round(q + (cx, cy), 3)


def text_lines(rng, shape, n_lines, size, step, kind='axis', margin=2):
    """chars along horizontal lines: char width ~size, advance step * width (< 1 overlaps, 1 touches)"""
    h, w = shape
    out = []
    for li in range(n_lines):
        ch = rng.uniform(size[0], size[1])
        cy = margin + ch / 2 + (h - 2 * margin - ch) * (li + 0.5) / n_lines
        x = margin + ch / 2
        while x + ch / 2 < w - margin:
            out.append(quad(x, cy + rng.uniform(-1, 1), ch * rng.uniform(0.8, 1.0), ch, kind, rng))
            x += ch * step * rng.uniform(0.9, 1.0)
    q = np.asarray(out, np.float64).reshape(-1, 4, 2)
    q[:, :, 0] = np.clip(q[:, :, 0], 0, w - 1)
    q[:, :, 1] = np.clip(q[:, :, 1], 0, h - 1)
    return q


def clipped(qs, shape):
    """quads clipped to the page (their boxes inside it)"""
    q = np.array(qs, np.float64).reshape(-1, 4, 2)
    q[:, :, 0] = np.clip(q[:, :, 0], 0, shape[1] - 1)
    q[:, :, 1] = np.clip(q[:, :, 1], 0, shape[0] - 1)
    return q


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

    def case(name, shape, qs, debug=False, **config):
        cfg = CharHeatmapDefaultEngineInitConfig(**{
            'gaussian_map_distance_factor': config.get('factor', 2.25),
            'gaussian_map_char_radius': config.get('radius', 25),
            'gaussian_map_preserving_score_min': config.get('preserving', 0.9),
            'weight_neutralized_score_map': config.get('weight', 0.4)})
        qs = np.asarray(qs, np.float64).reshape(-1, 4, 2)
        row = dict(name=name, shape=list(shape), debug=debug, factor=cfg.gaussian_map_distance_factor,
                   radius=cfg.gaussian_map_char_radius, preserving=cfg.gaussian_map_preserving_score_min,
                   weight=cfg.weight_neutralized_score_map, quads=put('f64', qs))
        engine = CharHeatmapDefaultEngine(cfg)
        try:
            result = engine.run(CharHeatmapEngineRunConfig(height=shape[0], width=shape[1], char_polygons=polygons_of(qs),
                                                           enable_debug=debug))
        except Exception as e:      # noqa: BLE001  (the reference's own exception is the expectation)
            row['raises'] = type(e).__name__
        else:
            row['score'] = put('f32', result.score_map.mat)
            if debug:
                for k in DEBUG_NAMES:
                    mat = getattr(result.debug, k).mat
                    row[k] = put('u8' if mat.dtype == np.uint8 else 'f32', mat)
        index.append(row)

    rng = default_rng(20261016)
    case('no-chars', (24, 32), np.zeros((0, 4, 2)))
    case('no-chars-debug', (24, 32), np.zeros((0, 4, 2)), debug=True)
    for kind in ('axis', 'rot', 'shear', 'persp'):
        for seed in range(2):
            case(f'one-{kind}-{seed}', (48, 64), [quad(rng.uniform(20, 44), rng.uniform(16, 32), rng.uniform(10, 24),
                                                       rng.uniform(10, 24), kind, rng)], debug=seed == 0)
    case('tiny-chars', (32, 40), [quad(rng.uniform(4, 36), rng.uniform(4, 28), rng.uniform(0.5, 4.5), rng.uniform(0.5, 4.5),
                                       k, rng) for k in ('axis', 'rot', 'persp', 'axis', 'shear', 'rot', 'axis', 'persp')])
    case('large-chars', (126, 124), clipped([quad(62, 63, 122, 124, 'axis', rng), quad(61, 62, 121, 123, 'persp', rng)], (126, 124)))
    for step in (1.0, 0.8, 0.6):
        for kind in ('axis', 'rot'):
            case(f'text-lines-{step}-{kind}', (56, 72), text_lines(rng, (56, 72), 3, (9, 16), step, kind), debug=kind == 'axis')
    base = [quad(20, 16, 14, 12, 'axis', rng), quad(40, 20, 12, 14, 'rot', rng)]
    case('duplicated', (40, 56), base + base + [base[0]], debug=True)
    case('collinear', (32, 32), [np.array([(4, 4), (12, 8), (20, 12), (28, 16)], np.float64)])
    case('collinear-vertical', (32, 32), [np.array([(10, 2), (10, 9), (10, 20), (10, 28)], np.float64)])
    case('point', (32, 32), [np.full((4, 2), 10.0), np.full((4, 2), 10.4)])
    case('bow-tie', (32, 40), [np.array([(4, 4), (30, 24), (30, 4), (4, 24)], np.float64)], debug=True)
    case('half-pixels', (32, 32), [np.array([(4.5, 4.5), (20.5, 5.5), (19.5, 21.5), (3.5, 20.5)], np.float64)])
    case('last-row-col', (30, 40), [np.array([(30, 20), (39, 20), (39, 29), (30, 29)], np.float64),
                                    np.array([(0, 25.4), (12, 25), (12, 29.4), (0, 29)], np.float64),
                                    clipped(quad(36, 14, 7, 9, 'rot', rng) + (2.4, 0), (30, 40))[0]])
    # a box not inside the page: the reference's exception
    sq = np.array([(0, 0), (9, 0), (9, 9), (0, 9)], np.float64)
    case('out-up', (30, 40), [sq + (5, 5), sq + (5, -2)])
    case('out-left', (30, 40), [sq + (-1, 5)])
    case('out-down-at-h', (30, 40), [sq + (5, 5), sq + (5, 21)])
    case('out-down-past-h', (30, 40), [sq + (5, 25)])
    case('out-right-at-w', (30, 40), [sq + (31, 5)])
    case('out-below', (30, 40), [sq + (5, 45)])
    case('out-page-shaped-at-h', (10, 10), [sq + (0, 1)])
    case('out-page-shaped-at-w', (10, 10), [sq + (1, 0)])
    case('out-second-of-three', (30, 40), [sq + (5, 5), sq + (35, 5), sq + (-3, 5)])
    # non-square pages and non-default configs
    case('wide', (24, 96), text_lines(rng, (24, 96), 1, (14, 18), 0.85, 'rot'))
    case('tall', (96, 24), clipped([quad(12, 9 + 16 * i, 16, 15, 'persp', rng) for i in range(6)], (96, 24)))
    qs = text_lines(rng, (48, 64), 2, (10, 18), 0.75, 'rot')
    for config in (dict(radius=5), dict(radius=40), dict(factor=1.0), dict(factor=3.5), dict(preserving=0.5),
                   dict(weight=0.0), dict(weight=0.25), dict(weight=1.0), dict(radius=40, factor=3.5, preserving=0.5, weight=1.0)):
        name = 'config-' + '-'.join(f'{k}{v}' for k, v in config.items())
        case(name, (48, 64), qs, debug=config in (dict(weight=0.25), dict(preserving=0.5)), **config)

    out = {k: np.concatenate(v) for k, v in packed.items()}
    out['index'] = np.array(json.dumps(index))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes,', len(index), 'cases,', sum('raises' in r for r in index), 'raising:',
          sorted({r['raises'] for r in index if 'raises' in r}))


if __name__ == '__main__':
    main()
