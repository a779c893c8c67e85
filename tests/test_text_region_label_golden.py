"""CPU checks of PageTextRegionLabelStep's specification: the numpy + oracle restatement (tests/text_region_label_restate.py)
against the reference's own runs (tests/golden/text_region_label.npz), the vectorised draws and validity the step uses, the
label class, the centroid restatement and the configs the step refuses."""
import math
import os
import sys

import numpy as np
import pytest
from numpy.random import default_rng

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_region_label_restate as R  # noqa: E402

CASES = R.load_golden()
ERRORS = {'AssertionError': AssertionError, 'ValueError': ValueError}
PLANES = ('char_mask', 'height', 'gaussian', 'box_mask')


def test_golden_covers_the_issue_cases():
    names = {c['name'] for c in CASES}
    assert len(CASES) >= 25
    assert {'scatter-axis', 'scatter-rot', 'scatter-shear', 'scatter-persp', 'overlapping'} <= names
    assert {c['num'] for c in CASES} >= {0, 1, 3}
    assert any(len(c['quads']) > 40 and c['name'].startswith('grid') for c in CASES)
    raising = {c['name']: c['raises'] for c in CASES if 'raises' in c}
    assert raising['small-box-height'] == raising['small-box-width'] == 'ValueError'
    assert raising['concave-candidate-outside'] == raising['box-past-the-page'] == 'AssertionError'
    assert sum(c['warnings'] for c in CASES) > 0


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_restatement_matches_the_reference_step(case):
    rng = default_rng(case['seed'])
    warnings = []
    args = (case['quads'], tuple(case['shape']), case['active'], rng, case['num'], case['factor'], warnings)
    if 'raises' in case:
        with pytest.raises(ERRORS[case['raises']]):
            R.run(*args)
    else:
        out = R.run(*args)
        for name in PLANES:
            assert out[name].dtype == case[name].dtype and out[name].tobytes() == case[name].tobytes(), name
        assert out['labels'] == R.golden_labels(case)
        assert len(warnings) == case['warnings']
    assert R.rng_state(rng) == case['rng_state']


def test_vectorised_draws_equal_the_scalar_sequence():
    """rng.integers(1, highs) over the interleaved bounds equals the reference's two scalar draws per candidate: values and
    the generator's final state"""
    from vkit_amd.pipeline.text_detection.page_text_region_label import draw_highs
    bounds = default_rng(7)
    for trial in range(40):
        n, m = int(bounds.integers(1, 60)), int(bounds.integers(1, 10))
        hw = bounds.integers(3, [8, 300][trial % 2], (n, 2))
        a, b = default_rng(trial), default_rng(trial)
        vec = a.integers(1, draw_highs(hw, m))
        scalar = [int(b.integers(1, hb)) for bh, bw in hw.tolist() for _ in range(m) for hb in (bh - 1, bw - 1)]
        assert vec.tolist() == scalar
        assert a.bit_generator.state == b.bit_generator.state


def _fma(a, b, c):
    from fractions import Fraction
    return float(Fraction(a) * Fraction(b) + Fraction(c))


@pytest.mark.parametrize('n', [1, 2, 3, 6])
def test_matmul_orders_of_affine_points(n):
    """the sums k_region_label_deviate writes for affine_points' np.matmul(H, (x, y, 1) columns): fma(a2, 1, fma(a1, y, a0 x))
    over two or more columns, fma(a2, 1, fma(a0, x, a1 y)) for a single column"""
    rng = default_rng(n)
    for _ in range(200):
        H = rng.normal(0, 1, (3, 3)) * rng.choice([1e-3, 1.0, 1e3], (3, 3))
        pts = np.concatenate((rng.integers(1, 200, (2, n)).astype(np.float32), np.ones((1, n), np.float32)))
        got = np.matmul(H, pts)
        for i in range(3):
            a0, a1, a2 = H[i].tolist()
            for j in range(n):
                x, y = float(pts[0, j]), float(pts[1, j])
                want = _fma(a2, 1.0, _fma(a0, x, a1 * y)) if n == 1 else _fma(a2, 1.0, _fma(a1, y, a0 * x))
                assert got[i, j] == want


def test_vectorised_validity_equals_the_scalar_one():
    from vkit_amd.pipeline.text_detection.page_text_region_label import labels_valid
    rng = default_rng(3)
    quads = np.concatenate([c['quads'] for c in CASES if c['quads'].ndim == 3 and c['quads'].shape[1:] == (4, 2)])
    k = np.arange(len(quads)).repeat(30)
    lo, hi = quads.min(axis=1)[k], quads.max(axis=1)[k]
    points = lo + (hi - lo) * rng.uniform(-0.2, 1.2, (len(k), 2))
    points[::7] = np.round(points[::7])                 # integer-valued label points too
    got = labels_valid(points[:, 1], points[:, 0], quads[k])
    want = [R.label_valid(float(y), float(x), quads[i]) for (x, y), i in zip(points.tolist(), k.tolist())]
    assert got.tolist() == want
    assert 0 < sum(want) < len(want)


def test_label_class_behaves_as_recorded():
    from vkit_amd.element import Point
    from vkit_amd.pipeline.text_detection import PageCharRegressionLabel, PageCharRegressionLabelTag as Tag
    checked = 0
    for case in (c for c in CASES if 'raises' not in c):
        labels = []
        for (c, t, sy, sx, iy, ix) in R.golden_labels(case):
            corners = [Point.create(y=y, x=x) for x, y in case['quads'][c].tolist()]
            labels.append(PageCharRegressionLabel(char_idx=c, tag=Tag.DEVIATE if t else Tag.CENTROID, label_point_smooth_y=sy,
                                                  label_point_smooth_x=sx, downsampled_label_point_y=iy,
                                                  downsampled_label_point_x=ix, up_left=corners[0], up_right=corners[1],
                                                  down_right=corners[2], down_left=corners[3]))
        assert [lb.valid for lb in labels] == case['label_valid'].astype(bool).tolist()
        assert [lb.bounding_orientation_idx for lb in labels] == case['label_orientation'].tolist()
        assert np.array([lb.generate_up_left_offsets() for lb in labels]).reshape(-1, 2).tobytes() == \
            case['label_offsets'].tobytes()
        assert np.array([lb.generate_clockwise_angle_distribution() for lb in labels]).reshape(-1, 4).tobytes() == \
            case['label_angles'].tobytes()
        assert np.array([lb.generate_clockwise_distances() for lb in labels]).reshape(-1, 4).tobytes() == \
            case['label_distances'].tobytes()
        few = [lb for lb in labels if lb.valid][:3]
        dy, dx = case['shift']
        shifted = [lb.to_shifted_page_char_regression_label(offset_y=dy, offset_x=dx) for lb in few]
        rows = [(s.label_point_smooth_y, s.label_point_smooth_x, s.downsampled_label_point_y, s.downsampled_label_point_x,
                 s.up_left.smooth_y, s.up_left.smooth_x, s.down_right.smooth_y, s.down_right.smooth_x, s.bounding_smooth_up,
                 s.bounding_smooth_left, float(s.valid)) for s in shifted]
        assert np.array(rows, np.float64).reshape(-1, 11).tobytes() == case['shifted'].tobytes()
        down = [lb.to_downsampled_page_char_regression_label(case['factor_down']) for lb in few]
        rows = [(d.downsampled_label_point_y, d.downsampled_label_point_x, float(d.is_downsampled),
                 d.downsample_labeling_factor, d.label_point_smooth_y, d.label_point_smooth_x) for d in down]
        assert np.array(rows, np.float64).reshape(-1, 6).tobytes() == case['downsampled'].tobytes()
        for d in down:
            with pytest.raises(AssertionError):
                d.to_shifted_page_char_regression_label(offset_y=1, offset_x=1)
            with pytest.raises(AssertionError):
                d.to_downsampled_page_char_regression_label(2)
        checked += len(labels)
    assert checked > 300


def test_copy_keeps_only_the_non_bounding_fields():
    from vkit_amd.element import Point
    from vkit_amd.pipeline.text_detection import PageCharRegressionLabel, PageCharRegressionLabelTag as Tag
    p = [Point.create(y=y, x=x) for x, y in [(0, 0), (10, 0), (10, 6), (0, 6)]]
    label = PageCharRegressionLabel(char_idx=0, tag=Tag.CENTROID, label_point_smooth_y=3.0, label_point_smooth_x=5.0,
                                    downsampled_label_point_y=3, downsampled_label_point_x=5, up_left=p[0], up_right=p[1],
                                    down_right=p[2], down_left=p[3])
    assert label.valid and label.bounding_orientation_idx == 1
    plain = label.copy()
    assert plain._valid is None and plain._up_left_vector is None and plain._bounding_smooth_up is None
    rich = label.copy(with_non_bounding_related_lazy_fields=True)
    assert rich._valid is True and rich._up_left_vector is label._up_left_vector and rich._bounding_smooth_up is None
    assert rich.generate_clockwise_distances() == label.generate_clockwise_distances()


def test_polygon_measures():
    from vkit_amd.element import Polygon
    q = np.array([(1.25, 2.5), (11.75, 3.0), (12.0, 9.5), (0.5, 8.75)])
    p = Polygon.from_smooth_xy(q)
    (ulx, uly), (urx, ury), (drx, dry), (dlx, dly) = q.tolist()
    assert p.get_rectangular_height() == (math.hypot(uly - dly, ulx - dlx) + math.hypot(ury - dry, urx - drx)) / 2
    c = p.get_center_point()
    # the polygon centroid by the shoelace formula, to rounding
    x, y = q[:, 0], q[:, 1]
    cross = x * np.roll(y, -1) - np.roll(x, -1) * y
    area = cross.sum() / 2
    assert abs(c.smooth_x - ((x + np.roll(x, -1)) * cross).sum() / (6 * area)) < 1e-12
    assert abs(c.smooth_y - ((y + np.roll(y, -1)) * cross).sum() / (6 * area)) < 1e-12
    # orientation does not change a bit of it; a zero-area ring takes the segment mid points, a point its first vertex
    assert Polygon.from_smooth_xy(q[::-1]).get_center_point().smooth_x == c.smooth_x
    line = Polygon.from_smooth_xy(np.array([(0, 0), (4, 0), (10, 0), (4, 0)], np.float64)).get_center_point()
    assert (line.smooth_x, line.smooth_y) == (5.0, 0.0)
    point = Polygon.from_smooth_xy(np.full((4, 2), 3.5)).get_center_point()
    assert (point.smooth_x, point.smooth_y) == (3.5, 3.5)


def test_external_ellipse_config_is_refused():
    from vkit_amd.pipeline.text_detection import page_text_region_label_step_factory as F
    with pytest.raises(NotImplementedError, match='char_bounding_polygons'):
        F.create({'char_mask_engine_config': {'type': 'external_ellipse'}})
    with pytest.raises(NotImplementedError):
        F.create({'char_mask_engine_config': {'type': 'nonexistent'}})
    with pytest.raises(ValueError):
        F.create({'char_heatmap_default_engine_init_config': {'gaussian_map_char_radius': 0}})
    assert F.create().config.num_deviate_char_regression_labels == 1


def test_box_fill_plan_follows_box_fill_mask():
    from vkit_amd.pipeline.text_detection.page_text_region_label import box_fill_plan
    assert box_fill_plan(2, 5, 3, 7, (10, 10)) == (None, (2, 5, 3, 7))
    assert box_fill_plan(2, 10, 3, 10, (10, 10)) == (None, (2, 9, 3, 9))          # ends one past the page: clipped
    assert isinstance(box_fill_plan(-1, 5, 3, 7, (10, 10))[0], AssertionError)
    assert isinstance(box_fill_plan(2, 11, 3, 7, (10, 10))[0], AssertionError)
    assert box_fill_plan(-1, 8, -1, 8, (10, 10)) == (None, (0, 9, 0, 9))          # the page's shape: the whole page
    assert box_fill_plan(10, 10, 3, 7, (10, 10)) == (None, None)                   # starts at the end: writes nothing
