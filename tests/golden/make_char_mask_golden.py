#!/usr/bin/env python3
"""Regenerates tests/golden/char_mask.npz by running THE REFERENCE's own external_ellipse char-mask engine
(vkit/engine/char_mask/external_ellipse.py) and PageDistortionStep.generate_char_labelings with that engine on small
synthetic pages.

    python tests/golden/make_char_mask_golden.py

The missing third-party modules are stubbed exactly as make_golden.py stubs them (it is imported for that).  Two cv2 calls
are oracle-patched: cv.getPerspectiveTransform becomes oracle.get_perspective_transform, and cv.warpPerspective becomes
oracle.warp_perspective behind cv2's rule that a dsize with a zero side means the source size (a sub-pixel quad asks for
one).  The engine is built directly from its init config.  Everything else -- the template, affine_np_points, the
placement and the trim, the fills and the exceptions -- is the reference's code running for real.

Stored per case, in one JSON ``index`` row: L, the page shape, where the quads (float64), bounding boxes, heights and the
expected outputs sit in a few flat arrays, and the exception type for the raising cases.  Data only.
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
from vkit.element import Box, Image, Point, PointList, Polygon  # noqa: E402
from vkit.engine.char_mask.external_ellipse import (  # noqa: E402
    CharMaskExternalEllipseEngine, CharMaskExternalEllipseEngineInitConfig)
from vkit.engine.char_mask.type import CharMaskEngineRunConfig  # noqa: E402
from vkit.engine.interface import EngineExecutor  # noqa: E402
from vkit.pipeline.text_detection import page_distortion as PD  # noqa: E402

OUT = os.path.join(HERE, 'char_mask.npz')


def _warp(src, M, dsize, *args, **kwargs):
    w, h = int(dsize[0]), int(dsize[1])
    if w <= 0 or h <= 0:
        h, w = src.shape[:2]
    return O.warp_perspective(src, M, (w, h))


cv_stub.getPerspectiveTransform = lambda a, b, *rest: O.get_perspective_transform(a, b)
cv_stub.warpPerspective = _warp


def quads(rng, n, shape, size, kind, spread=0.0, margin=0):
    """n quads (n, 4, 2) float64 (x, y) of side ~size: kind 'axis', 'rot', 'shear' or 'persp'; centres over the page grown
    by ``spread`` of its size on every side (edge-crossing and off-page chars), or shrunk by ``margin`` px."""
    h, w = shape
    out = []
    for _ in range(n):
        s = rng.uniform(size[0], size[1])
        cx = rng.uniform(-spread * w + margin, w * (1 + spread) - margin)
        cy = rng.uniform(-spread * h + margin, h * (1 + spread) - margin)
        sq = np.array([(-1, -1), (1, -1), (1, 1), (-1, 1)], np.float64) * s / 2
        if kind in ('rot', 'shear', 'persp'):
            a = rng.uniform(-0.6, 0.6)
            rot = np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]])
            sq = sq @ rot.T
        if kind in ('shear', 'persp'):
            sq = sq @ np.array([[1, rng.uniform(-0.4, 0.4)], [rng.uniform(-0.3, 0.3), 1]]).T
        if kind == 'persp':
            sq = sq + rng.uniform(-0.2, 0.2, (4, 2)) * s
        out.append(sq + (cx, cy))
    return np.round(np.asarray(out), 3)


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

    def engine_case(name, L, shape, qs, bounds=None):
        engine = CharMaskExternalEllipseEngine(CharMaskExternalEllipseEngineInitConfig(internal_side_length=L))
        boxes = [Box(up=int(b[0]), down=int(b[1]), left=int(b[2]), right=int(b[3])) for b in bounds] if bounds is not None else None
        row = dict(name=name, kind='engine', L=L, shape=list(shape), quads=put('f64', np.asarray(qs, np.float64).reshape(-1, 4, 2)))
        if bounds is not None:
            row['bounds'] = put('i32', np.asarray(bounds, np.int32).reshape(-1, 4))
        try:
            result = engine.run(CharMaskEngineRunConfig(height=shape[0], width=shape[1], char_polygons=polygons_of(qs),
                                                        char_bounding_boxes=boxes))
        except Exception as e:      # noqa: BLE001  (the reference's own exception is the expectation)
            row['raises'] = type(e).__name__
        else:
            row['combined'] = put('u8', result.combined_chars_mask.mat)
            row['boxes'] = put('i32', np.asarray([(m.box.up, m.box.down, m.box.left, m.box.right) for m in result.char_masks],
                                                 np.int32).reshape(-1, 4))
            row['char_masks'] = put('u8', np.concatenate([m.mat.reshape(-1) for m in result.char_masks]) if result.char_masks
                                    else np.zeros(0, np.uint8))
        index.append(row)

    rng = default_rng(20261015)
    page = (96, 128)
    for L in (40, 20, 33, 64):
        for kind in ('axis', 'rot', 'shear', 'persp'):
            for seed in range(2):
                # discs on the page (one wholly off it raises: covered below)
                engine_case(f'inside-{L}-{kind}-{seed}', L, page, quads(rng, 12, page, (4, 26), kind, margin=30))
    for L in (40, 20):
        for kind in ('axis', 'persp'):
            for seed in range(3):
                # chars near the page edges: discs clipped by the edge, some wholly outside (raising cases keep going)
                qs = quads(rng, 10, page, (6, 30), kind, spread=0.08)
                engine_case(f'edge-{L}-{kind}-{seed}', L, page, qs)
    # named edge behaviour
    sq = np.array([(0, 0), (19, 0), (19, 19), (0, 19)], np.float64)
    engine_case('clipped-top', 20, (100, 100), [sq + (40, -5)])
    engine_case('clipped-left-bottom', 40, (100, 100), [sq * 2 + (-20, 70)])
    engine_case('off-page-right', 20, (100, 100), [sq + (130, 10)])
    engine_case('off-page-below', 33, (100, 100), [sq + (10, 140)])
    engine_case('sub-pixel', 40, (100, 100), [np.array([(10, 10), (10.4, 10), (10.4, 19), (10, 19)], np.float64)])
    engine_case('point', 20, (100, 100), [np.full((4, 2), 10.0)])
    engine_case('flat', 20, (100, 100), [np.array([(10, 10), (30, 10), (30, 10), (10, 10)], np.float64)])
    engine_case('half-pixel', 20, (64, 64), [sq * 0.5 + (20.5, 20.5), sq * 0.5 + (31.5, 9.5)])
    # bounding boxes
    for L in (40, 64):
        qs = quads(rng, 8, page, (8, 24), 'rot', margin=30)
        b = []
        for q in qs:
            cy, cx = q[:, 1].mean(), q[:, 0].mean()
            b.append((max(0, int(cy) - 12), min(page[0] - 1, int(cy) + 9), max(0, int(cx) - 10), min(page[1] - 1, int(cx) + 14)))
        engine_case(f'bounds-{L}', L, page, qs, np.asarray(b))

    # the step's char labels with the ellipse engine: char mask, seal-impression char mask, height map (ties included)
    for seed, L in ((0, 40), (1, 20), (2, 33)):
        qs = quads(rng, 30, page, (6, 20), 'persp', margin=30)
        seal = quads(rng, 6, page, (6, 16), 'rot', margin=30)
        up = rng.uniform(10, 80, (30, 2)).round(1)
        down = up + rng.integers(1, 5, (30, 1)) * np.array([[0.0, 3.0]])       # heights with ties
        config = PD.PageDistortionStepConfig(char_mask_engine_config={'type': 'external_ellipse',
                                                                      'config': {'internal_side_length': L}})
        step = PD.PageDistortionStep.__new__(PD.PageDistortionStep)
        step.config = config
        step.char_mask_engine_executor = EngineExecutor(
            CharMaskExternalEllipseEngine(CharMaskExternalEllipseEngineInitConfig(internal_side_length=L)))
        image = Image(mat=np.zeros(page + (3,), np.uint8))
        pts_up = PointList(Point.create(y=float(y), x=float(x)) for x, y in up)
        pts_down = PointList(Point.create(y=float(y), x=float(x)) for x, y in down)
        char_mask, seal_mask, height_map, heights, _ = step.generate_char_labelings(
            image, polygons_of(qs), polygons_of(seal), pts_up, pts_down)
        index.append(dict(name=f'labels-{seed}', kind='labels', L=L, shape=list(page), quads=put('f64', qs), seal=put('f64', seal),
                          up=put('f64', up), down=put('f64', down), char_mask=put('u8', char_mask.mat),
                          seal_mask=put('u8', seal_mask.mat), height_map=put('f32', height_map.mat),
                          heights=put('f64', np.asarray(heights))))

    out = {k: np.concatenate(v) for k, v in packed.items()}
    out['index'] = np.array(json.dumps(index))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes,', len(index), 'cases,', sum('raises' in r for r in index), 'raising:',
          sorted({r['raises'] for r in index if 'raises' in r}))


if __name__ == '__main__':
    main()
