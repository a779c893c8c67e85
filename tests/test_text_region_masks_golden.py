"""tests/golden/text_region_masks.npz (the reference's own TextRegionFlattener.get_bounding_extended_text_region_masks and
Polygon.to_bounding_rectangular_polygon, see tests/golden/make_text_region_masks_golden.py) against the numpy restatement that
the GPU tests compare with (tests/text_region_masks_restate.py) -- this pins the closed form of the mask algebra -- and against
the host mirror of the rectangle in vkit_amd/element/polygon.py.  No GPU.  Every comparison is exact."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_region_masks_restate as R  # noqa: E402

RUNS, RECTANGLES = R.load_golden()


def polygon_of(points):
    from vkit_amd.element import Polygon
    return Polygon.from_xy_pairs([(int(x), int(y)) for x, y in points])


def points_of(polygon):
    return np.array([(p.x, p.y) for p in polygon.points], np.int32)


def test_the_golden_holds_the_cases():
    assert len(RUNS) == 36 and {(tuple(r['shape']), r['n']) for r in RUNS} == {(s, n) for s in R.PAGES for n in R.COUNTS}
    assert {bool(r['typical']) for r in RUNS} == {False, True}
    shapes = {m['mat'].shape for r in RUNS for m in r['masks']}
    assert (1, 1) in shapes and any(h == 1 and w > 1 for h, w in shapes) and any(w == 1 and h > 1 for h, w in shapes)
    counts = {len(g['original']) for r in RUNS for g in r['regions']}
    assert {1, 2, 3, 48, 68} <= counts
    assert {r['angles'][k] for r in RUNS for k, g in enumerate(r['regions']) if g['patched'] is not None} == set(R.ANGLES)
    # a neighbour's rectangle over another region's polygon: somewhere `r and T and not o` trims a dilated polygon
    run = next(r for r in RUNS if r['n'] == 3 and not r['typical'])
    o, d, r = (run['regions'][2][k] for k in ('original', 'dilated', 'rectangle'))
    box = R.union_box(R.bounding_box(d), R.bounding_box(r))
    T = R.text_mask(run['shape'], [g['original'] for g in run['regions']])[box[0]:box[1] + 1, box[2]:box[3] + 1]
    assert (R.placed(r, box) & T & ~R.placed(o, box) & R.placed(d, box)).any()


@pytest.mark.parametrize('k', range(len(RUNS)))
def test_restatement_against_the_golden(k):
    run = RUNS[k]
    rectangles = [g['rectangle'] if g['patched'] is None else g['patched'] for g in run['regions']]
    got = R.extended_masks(run['shape'], [g['original'] for g in run['regions']], [g['dilated'] for g in run['regions']], rectangles)
    assert len(got) == len(run['masks']) == run['n']
    for (mat, box), want in zip(got, run['masks']):
        assert list(box) == want['box']
        assert mat.dtype == want['mat'].dtype == np.uint8 and mat.shape == want['mat'].shape
        assert mat.tobytes() == want['mat'].tobytes()


def test_patched_rectangles_against_the_golden():
    seen = 0
    for run in RUNS:
        for g, angle in zip(run['regions'], run['angles']):
            if g['patched'] is not None:
                got = points_of(polygon_of(g['dilated']).to_bounding_rectangular_polygon(shape=tuple(run['shape']), angle=angle))
                assert got.tolist() == g['patched'].tolist()
                seen += 1
    assert seen > 100


def test_direct_rectangles_against_the_golden():
    assert len(RECTANGLES) == 336
    for row in RECTANGLES:
        got = polygon_of(row['points']).to_bounding_rectangular_polygon(tuple(row['shape']), row['angle'])
        assert got.num_points == 4 and points_of(got).tolist() == row['rectangle'].tolist(), row


def test_intersection_errors_and_the_minimum_rectangle():
    from vkit_amd.element import Polygon
    with pytest.raises(RuntimeError, match='Lines are vertical.'):
        Polygon.calculate_lines_intersection_point(np.zeros(2), np.pi / 2, np.ones(2), np.pi / 2)
    with pytest.raises(RuntimeError, match='Lines not intersected.'):
        Polygon.calculate_lines_intersection_point(np.zeros(2), 0.3, np.array([0.0, 1.0]), 0.3)
    point = Polygon.calculate_lines_intersection_point(np.array([2.0, 0.0]), np.pi / 2, np.array([0.0, 3.0]), 0.0)
    assert (point.smooth_x, point.smooth_y) == (2.0, 3.0)
    begin, end = Polygon.project_polygon_to_unit_vector(np.array([(1.0, 5.0), (4.0, -2.0)]), 0.0)
    assert begin.tolist() == [1.0, 0.0] and end.tolist() == [4.0, 0.0]
    with pytest.raises(NotImplementedError, match='outside the accelerated path'):
        polygon_of([(1, 1), (9, 2), (8, 7)]).to_bounding_rectangular_polygon((20, 20))
