"""CPU checks of char binding: the numpy restatement (tests/char_binding_restate.py) against the reference's own runs
(tests/golden/char_binding.npz), and the host half of the binding -- the batched self-relative tables, the envelope pairs and
the split plan of vkit_amd/pipeline/text_detection/page_text_region.py -- against the per-polygon properties and the
restatement.  Every comparison is exact."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import char_binding_restate as R  # noqa: E402

GOLDEN_RUNS = R.load_golden()
ALL_CASES = [(kind, seed) for kind in R.KINDS for seed in (0, 1, 2)]


def polygon_of(points):
    from vkit_amd.element import Polygon
    return Polygon.from_xy_pairs([(float(x), float(y)) for x, y in points])


def test_the_golden_covers_every_kind():
    assert [(run['kind'], run['seed']) for run in GOLDEN_RUNS] == [(kind, seed) for kind in R.KINDS for seed in R.GOLDEN_SEEDS]
    for run in GOLDEN_RUNS:
        anchors, candidates = R.make_case(run['seed'], run['kind'])
        assert len(anchors) == len(run['anchors']) and len(candidates) == len(run['candidates'])
        for made, stored in zip(anchors + candidates, run['anchors'] + run['candidates']):
            assert made.tobytes() == stored.tobytes()


@pytest.mark.parametrize('k', range(len(GOLDEN_RUNS)))
def test_restatement_equals_the_golden(k):
    run = GOLDEN_RUNS[k]
    case = R.Case(run['anchors'], run['candidates'])
    pairs, counts = case.pairs()
    assert pairs == [tuple(p) for p in run['pairs'].tolist()]
    assert counts == [tuple(c) for c in run['counts'].tolist()]
    assert np.array(case.ratios(True), np.float64).tobytes() == run['ratio'].tobytes()
    assert np.array(case.ratios(False), np.float64).tobytes() == run['ratio_union'].tobytes()
    assert case.bind() == run['bound'].tolist()
    assert case.infos() == run['infos']


def test_the_golden_holds_the_cases_the_binding_turns_on():
    by_kind = {(run['kind'], run['seed']): run for run in GOLDEN_RUNS}
    binding = by_kind[('binding', 0)]
    assert binding['bound'].tolist() == [0, 3, -1, -1, 7, 7, 7]                 # the lower of equal ratios; the second of three
    assert binding['infos'] == [(0, [0]), (3, [1]), (7, [4, 5, 6])]             # regions 1, 2, 4, 5, 6 received no char
    assert (2, 5) in [tuple(p) for p in binding['pairs'].tolist()]              # met, ratio 0.0: yielded, not bound
    envelope = by_kind[('envelope', 0)]
    pairs = [tuple(p) for p in envelope['pairs'].tolist()]
    assert (0, 0) in pairs and (4, 0) in pairs                                  # touching on one column / one row
    assert not [p for p in pairs if p[0] in (1, 5)]                             # one pixel apart; far away
    assert envelope['counts'][pairs.index((2, 2))].tolist()[0] == 0             # envelopes overlap, no shared pixel
    nested = envelope['counts'][pairs.index((3, 3))].tolist()
    assert nested[0] == nested[2]                                               # nested: all of the candidate


@pytest.mark.parametrize('kind,seed', ALL_CASES)
def test_batched_tables_equal_the_polygon_properties(kind, seed):
    """Polygon.bounding_box and Polygon.self_relative_polygon.to_np_array() of every polygon, value for value; float points
    ending in .5, negative coordinates and a closing duplicate are among the 'raster' polygons"""
    from vkit_amd.pipeline.text_detection import polygon_overlap_tables
    anchors, candidates = R.make_case(seed, kind)
    polygons = [polygon_of(p) for p in anchors + candidates]
    records, points, envelopes = polygon_overlap_tables(polygons)
    assert points.dtype == np.int32 and envelopes.shape == (len(polygons), 4)
    for rec, polygon, smooth, env in zip(records, polygons, anchors + candidates, envelopes.tolist()):
        box = polygon.bounding_box
        assert (int(rec['up']), int(rec['left']), int(rec['h']), int(rec['w'])) == (box.up, box.left, box.height, box.width)
        want = polygon.self_relative_polygon.to_np_array()
        got = points[int(rec['pts_off']):int(rec['pts_off']) + int(rec['pts_cnt'])]
        assert got.shape == want.shape and (got == want).all()
        # ... and both equal the restatement's
        r_box, r_points = R.self_relative(smooth)
        assert (box.up, box.down, box.left, box.right) == r_box and (want == r_points).all()
        xy = np.array(polygon.to_xy_pairs(), np.int64)
        assert tuple(env) == (xy[:, 0].min(), xy[:, 0].max(), xy[:, 1].min(), xy[:, 1].max()) == R.envelope(smooth)


def test_tables_meet_half_points_negative_points_and_a_closing_duplicate():
    anchors, _ = R.make_case(0, 'raster')
    flat = np.concatenate(anchors)
    assert (flat % 1 == 0.5).any() and (flat < 0).any()
    assert any(len(p) > 2 and (R.int_points(p)[0] == R.int_points(p)[-1]).all() for p in anchors)
    assert any(len(R.self_relative(p)[1]) == len(p) - 1 for p in anchors)
    assert {len(p) for p in anchors} >= {1, 2, 3, 68}


@pytest.mark.parametrize('kind,seed', ALL_CASES)
def test_envelope_pairs_equal_the_restated_query(kind, seed):
    from vkit_amd.pipeline.text_detection import envelope_pairs
    anchors, candidates = R.make_case(seed, kind)
    got = envelope_pairs(np.array([R.envelope(p) for p in anchors]), np.array([R.envelope(p) for p in candidates]))
    want = [(c, a) for c in range(len(candidates)) for a in range(len(anchors))
            if R.envelopes_meet(R.envelope(anchors[a]), R.envelope(candidates[c]))]
    assert got.dtype == np.int32 and got.tolist() == [list(p) for p in want]


def test_envelope_pairs_without_polygons():
    from vkit_amd.pipeline.text_detection import envelope_pairs
    assert envelope_pairs(np.zeros((0, 4)), np.zeros((3, 4))).shape == (0, 2)
    assert envelope_pairs(np.zeros((3, 4)), np.zeros((0, 4))).shape == (0, 2)


def test_split_plan_keeps_candidates_whole_and_within_the_bound():
    from vkit_amd.pipeline.text_detection.page_text_region import plan_overlap_calls
    pairs = np.array([(0, 0), (0, 1), (1, 1), (2, 0), (2, 2), (4, 2)], np.int32)
    anchor_bytes, candidate_bytes = np.array([100, 200, 300]), np.array([10, 20, 30, 40, 50])
    assert plan_overlap_calls(pairs, anchor_bytes, candidate_bytes, 10 ** 6) == [(0, 6)]
    assert plan_overlap_calls(pairs, anchor_bytes, candidate_bytes, 710) == [(0, 6)]          # 600 + 10 + 20 + 30 + 50
    assert plan_overlap_calls(pairs, anchor_bytes, candidate_bytes, 709) == [(0, 5), (5, 6)]
    assert plan_overlap_calls(pairs, anchor_bytes, candidate_bytes, 330) == [(0, 3), (3, 5), (5, 6)]
    assert plan_overlap_calls(pairs, anchor_bytes, candidate_bytes, 1) == [(0, 2), (2, 3), (3, 5), (5, 6)]


def test_nothing_new_imports_shapely_or_torch():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for path in ('vkit_amd/pipeline/text_detection/page_text_region.py', 'vkit_amd/_native.py'):
        text = open(os.path.join(root, path)).read()
        assert not re.search(r'^\s*(import|from)\s+(shapely|torch)\b', text, flags=re.M), path
