"""Pins the envelope rule of char binding (tests/char_binding_restate.py: envelopes_meet; vkit_amd's envelope_pairs) against a
real shapely STRtree -- only where shapely is installed.

The build image has no shapely, so this test is skipped there and the rule stays a restatement of shapely's documented
behaviour.  Where shapely imports: ``sorted(STRtree(anchors).query(candidate))`` without a predicate,
the geometries built as the reference builds them, ``ShapelyPolygon(polygon.to_xy_pairs())``, on the cases of make_case.
Polygons of fewer than three points are left out: shapely does not build them."""
import os
import sys

import numpy as np
import pytest

pytest.importorskip('shapely')
from shapely.geometry import Polygon as ShapelyPolygon  # noqa: E402
from shapely.strtree import STRtree  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import char_binding_restate as R  # noqa: E402


@pytest.mark.parametrize('kind', R.KINDS)
def test_the_envelope_rule_is_the_tree_query(kind):
    from vkit_amd.pipeline.text_detection import envelope_pairs
    anchors, candidates = R.make_case(0, kind)
    anchors = [p for p in anchors if len(p) >= 3]
    candidates = [p for p in candidates if len(p) >= 3]
    geometries = [ShapelyPolygon([tuple(xy) for xy in R.int_points(p).tolist()]) for p in anchors]
    tree = STRtree(geometries)
    index_of = {id(g): k for k, g in enumerate(geometries)}
    want = []
    for c, points in enumerate(candidates):
        answers = tree.query(ShapelyPolygon([tuple(xy) for xy in R.int_points(points).tolist()]))
        # (shapely 2 answers indices, shapely 1 the geometries themselves)
        answers = sorted(int(a) if isinstance(a, (int, np.integer)) else index_of[id(a)] for a in answers)
        assert answers == [a for a in range(len(anchors)) if R.envelopes_meet(R.envelope(anchors[a]), R.envelope(points))]
        want += [[c, a] for a in answers]
    got = envelope_pairs(np.array([R.envelope(p) for p in anchors]).reshape(-1, 4),
                         np.array([R.envelope(p) for p in candidates]).reshape(-1, 4))
    assert got.tolist() == want
