#!/usr/bin/env python3
"""Regenerates tests/golden/char_binding.npz by running THE REFERENCE's own calculate_boxed_masks_intersected_ratio
(vkit/pipeline/text_detection/page_text_region.py:189-227), PageTextRegionStep.strtree_query_intersected_polygons (:899-925)
and the char-binding loop of PageTextRegionStep.run (:1160-1216) on small synthetic pages:

    python tests/golden/make_char_binding_golden.py

The binding loop is a stretch of ``run``, which cannot be called without a whole pipeline: its lines are read from the
reference's module when this script runs (inspect.getsource) and executed over the names the stretch uses.  Nothing of it is
kept here.

The missing third-party modules are stubbed as make_golden.py stubs them (it is imported for that); cv.fillPoly is the
oracle's, as in make_text_region_flatten_golden.py.  shapely is absent: ``ShapelyPolygon`` is a stub that keeps the integer
points it is given, and ``STRtree`` a stub whose ``query(geometry)`` answers the indices of the geometries whose envelope
(closed integer rectangle of their points) meets the query's -- a RESTATEMENT of shapely's documented behaviour without a
predicate, not shapely itself (tests/test_shapely_strtree_optional.py compares the rule with a real STRtree where shapely
imports).

Cases (tests/char_binding_restate.py: make_case): the kinds 'seams', 'envelope', 'binding', 'raster' and 'page', two seeds
each.  Stored: the smooth point tables, the (candidate, anchor) pairs in the order the reference visits them, the three integer
counts of every pair (intersected, anchor and candidate area, taken from the masks the reference yields), the ratios with the
candidate as base (as yielded) and with the union as base (the function called directly), the bound region of every char and
the char index lists of the infos.  Data only, never reference source text.
"""
import inspect
import json
import logging
import os
import sys
import textwrap
import zipfile
from collections import defaultdict
from types import SimpleNamespace
from typing import DefaultDict, List

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402,F401  (stubs cv2 & co., puts the reference and this repository on sys.path)

sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

import cv2 as cv_stub  # noqa: E402  (the MagicMock)
import char_binding_restate as R  # noqa: E402
from make_text_region_flatten_golden import _fill_poly  # noqa: E402
import vkit.element.polygon as reference_polygon  # noqa: E402
from vkit.element import Polygon  # noqa: E402
from vkit.pipeline.text_detection import page_text_region as TR  # noqa: E402

OUT = os.path.join(HERE, 'char_binding.npz')
BINDING_LINES = (1160, 1216)        # of the reference's page_text_region.py, inside PageTextRegionStep.run


class ShapelyPolygonStub:
    def __init__(self, xy_pairs):
        xy = np.asarray(xy_pairs, np.int64).reshape(-1, 2)
        self.envelope = (int(xy[:, 0].min()), int(xy[:, 0].max()), int(xy[:, 1].min()), int(xy[:, 1].max()))


class STRtreeStub:
    def __init__(self, geometries):
        self.envelopes = [g.envelope for g in geometries]

    def query(self, geometry):
        c = geometry.envelope
        # (in no particular order, like the tree: the reference sorts)
        return [k for k in reversed(range(len(self.envelopes)))
                if self.envelopes[k][0] <= c[1] and c[0] <= self.envelopes[k][1]
                and self.envelopes[k][2] <= c[3] and c[2] <= self.envelopes[k][3]]


def binding_source():
    lines, first = inspect.getsourcelines(TR.PageTextRegionStep.run)
    begin, end = BINDING_LINES[0] - first, BINDING_LINES[1] - first + 1
    assert 0 <= begin < end <= len(lines)
    return textwrap.dedent(''.join(lines[begin:end]))


def polygon_of(points):
    return Polygon.from_xy_pairs([(float(x), float(y)) for x, y in points])


def main():
    cv_stub.fillPoly = _fill_poly
    reference_polygon.ShapelyPolygon = ShapelyPolygonStub
    TR.ShapelyPolygon = ShapelyPolygonStub
    TR.STRtree = STRtreeStub
    source = compile(binding_source(), 'binding loop of the reference', 'exec')
    step = SimpleNamespace(config=SimpleNamespace(use_adjusted_char_polygons=False),
                           strtree_query_intersected_polygons=TR.PageTextRegionStep.strtree_query_intersected_polygons)
    points, ints, floats, runs = [], [], [], []

    def put(store, array, dtype):
        array = np.ascontiguousarray(array, dtype=dtype)
        at = sum(a.size for a in store)
        store.append(array.reshape(-1))
        return [at, list(array.shape)]

    def put_points(tables):
        out = []
        for table in tables:
            out.append([sum(len(t) for t in points), len(table)])
            points.append(np.asarray(table, np.float64).reshape(-1, 2))
        return out

    for kind in R.KINDS:
        for seed in R.GOLDEN_SEEDS:
            anchors, candidates = R.make_case(seed, kind)
            anchor_polygons = [polygon_of(p) for p in anchors]
            candidate_polygons = [polygon_of(p) for p in candidates]
            tree = STRtreeStub([p.to_shapely_polygon() for p in anchor_polygons])
            pairs, counts, ratio, ratio_union = [], [], [], []
            for c, candidate_polygon in enumerate(candidate_polygons):
                for anchor_idx, anchor_polygon, anchor_mask, candidate_mask, intersected_ratio in \
                        TR.PageTextRegionStep.strtree_query_intersected_polygons(tree, anchor_polygons, candidate_polygon):
                    assert anchor_polygon is anchor_polygons[anchor_idx]
                    union_ratio = TR.calculate_boxed_masks_intersected_ratio(anchor_mask, candidate_mask)
                    anchor_area, candidate_area = int(anchor_mask.np_mask.sum()), int(candidate_mask.np_mask.sum())
                    # the intersected area out of the reference's two ratios: both are exact quotients of small integers
                    intersected_area = round(intersected_ratio * candidate_area)
                    assert intersected_area / candidate_area == intersected_ratio
                    assert union_ratio == intersected_area / (anchor_area + candidate_area - intersected_area)
                    pairs.append((c, anchor_idx))
                    counts.append((intersected_area, anchor_area, candidate_area))
                    ratio.append(intersected_ratio)
                    ratio_union.append(union_ratio)
            # the binding loop itself, over the names it reads
            names = dict(precise_text_region_candidate_polygons=anchor_polygons, self=step,
                         page_char_polygon_collection=SimpleNamespace(char_polygons=candidate_polygons), List=List,
                         DefaultDict=DefaultDict, defaultdict=defaultdict, Polygon=Polygon, ShapelyPolygon=ShapelyPolygonStub,
                         STRtree=STRtreeStub, PageTextRegionInfo=TR.PageTextRegionInfo, logger=logging.getLogger('golden'))
            exec(source, names)
            region_index = {id(p): k for k, p in enumerate(anchor_polygons)}
            char_index = {id(p): k for k, p in enumerate(candidate_polygons)}
            infos = [[region_index[id(info.precise_text_region_polygon)], [char_index[id(p)] for p in info.char_polygons]]
                     for info in names['page_text_region_infos']]
            bound = np.full(len(candidates), -1, np.int64)
            for a, chars in infos:
                bound[chars] = a
            runs.append(dict(kind=kind, seed=seed, anchors=put_points(anchors), candidates=put_points(candidates),
                             pairs=put(ints, np.array(pairs, np.int64).reshape(-1, 2), np.int64),
                             counts=put(ints, np.array(counts, np.int64).reshape(-1, 3), np.int64),
                             bound=put(ints, bound, np.int64), ratio=put(floats, ratio, np.float64),
                             ratio_union=put(floats, ratio_union, np.float64), infos=infos))
    # an .npz with fixed member times (np.savez stamps the clock): the file regenerates byte for byte
    arrays = dict(points=np.concatenate(points), int=np.concatenate(ints), float=np.concatenate(floats),
                  index=np.array(json.dumps(dict(runs=runs))))
    with zipfile.ZipFile(OUT, 'w', zipfile.ZIP_DEFLATED) as archive:
        for name, array in arrays.items():
            member = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            member.compress_type = zipfile.ZIP_DEFLATED
            with archive.open(member, 'w') as f:
                np.lib.format.write_array(f, array, allow_pickle=False)
    print(OUT, os.path.getsize(OUT), 'bytes', len(runs), 'runs', sum(r['pairs'][1][0] for r in runs), 'pairs')


if __name__ == '__main__':
    main()
