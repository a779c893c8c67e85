"""CPU checks of the default char-heatmap engine's specification: the numpy + oracle restatement
(tests/char_heatmap_restate.py) against the reference's own runs (tests/golden/char_heatmap.npz), the package's host
template, the executor factory, the configs it refuses and the range bound those refusals rest on."""
import os
import sys

import numpy as np
import pytest
from numpy.random import default_rng

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import char_heatmap_restate as R  # noqa: E402

CASES = R.load_golden()
ERRORS = {'AssertionError': AssertionError, 'IndexError': IndexError}


def test_golden_covers_the_issue_cases():
    names = {c['name'] for c in CASES}
    assert {'no-chars', 'tiny-chars', 'large-chars', 'duplicated', 'collinear', 'point', 'bow-tie', 'last-row-col'} <= names
    assert {c.get('raises') for c in CASES} >= {None, 'AssertionError', 'IndexError'}
    assert {c['radius'] for c in CASES} >= {5, 25, 40} and {c['factor'] for c in CASES} >= {1.0, 2.25, 3.5}
    assert {c['weight'] for c in CASES} >= {0.0, 0.25, 0.4, 1.0} and 0.5 in {c['preserving'] for c in CASES}
    assert any(c['shape'][0] != c['shape'][1] for c in CASES)
    large = next(c for c in CASES if c['name'] == 'large-chars')
    assert (large['quads'].max(axis=1) - large['quads'].min(axis=1)).min() >= 120
    tiny = next(c for c in CASES if c['name'] == 'tiny-chars')
    assert (tiny['quads'].max(axis=1) - tiny['quads'].min(axis=1)).max() < 5
    debug = [c for c in CASES if c['debug'] and 'raises' not in c]
    # the neutralized branch below the preserving score really occurs
    assert any(((c['neutralized_mask'] > 0) & (c['score_map_max'] < c['preserving'])).any() for c in debug)


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_restatement_matches_the_reference_engine(case):
    shape = tuple(case['shape'])
    if 'raises' in case:
        with pytest.raises(ERRORS[case['raises']]):
            R.run(case['quads'], shape, **R.config_of(case))
        return
    out = R.run(case['quads'], shape, **R.config_of(case))
    assert out['score'].tobytes() == case['score'].tobytes()
    if case['debug']:
        for name in R.DEBUG_NAMES:
            assert out[name].dtype == case[name].dtype and out[name].tobytes() == case[name].tobytes(), name


def test_engine_box_exceptions_match_the_golden():
    """the engine raises the reference's exception from host data alone, before any launch"""
    from vkit_amd.element import Polygon
    from vkit_amd.engine.char_heatmap import char_heatmap_default_engine_executor_factory as F
    ex = F.create()
    for case in (c for c in CASES if 'raises' in c):
        h, w = case['shape']
        with pytest.raises(ERRORS[case['raises']]):
            ex.run({'height': h, 'width': w, 'char_polygons': [Polygon.from_smooth_xy(q) for q in case['quads']]})


@pytest.mark.parametrize('radius,factor', [(25, 2.25), (5, 2.25), (40, 2.25), (25, 1.0), (25, 3.5), (1, 0.3), (1024, 2.25)])
def test_host_template_equals_the_reference_expression(radius, factor):
    from vkit_amd.engine.char_heatmap import CharHeatmapDefaultEngine, CharHeatmapDefaultEngineInitConfig, build_np_distance
    engine = CharHeatmapDefaultEngine(CharHeatmapDefaultEngineInitConfig(gaussian_map_distance_factor=factor,
                                                                         gaussian_map_char_radius=radius))
    want, points = R.template(radius, factor)
    assert engine.np_gaussian_map.dtype == np.float32 and engine.np_gaussian_map.tobytes() == want.tobytes()
    assert np.array_equal(engine.np_char_points, points)
    assert build_np_distance(radius).dtype == np.float32


def test_factory_and_configs():
    from vkit_amd.engine.char_heatmap import (CharHeatmapDefaultEngine, CharHeatmapDefaultEngineInitConfig,
                                              CharHeatmapEngineRunConfig, char_heatmap_default_engine_executor_factory as F)
    assert F.get_type_name() == 'default' and CharHeatmapDefaultEngine.get_type_name() == 'default'
    ex = F.create()
    assert isinstance(ex.engine, CharHeatmapDefaultEngine) and ex.engine.init_config == CharHeatmapDefaultEngineInitConfig()
    c = ex.engine.init_config
    assert (c.gaussian_map_distance_factor, c.gaussian_map_char_radius, c.gaussian_map_preserving_score_min,
            c.weight_neutralized_score_map) == (2.25, 25, 0.9, 0.4)
    assert F.create({'gaussian_map_char_radius': 7}).engine.init_config.gaussian_map_char_radius == 7
    cfg = CharHeatmapDefaultEngineInitConfig(weight_neutralized_score_map=0.25)
    assert F.create(cfg).engine.init_config is cfg
    with pytest.raises(TypeError):
        F.create({'no_such_field': 1})
    assert CharHeatmapEngineRunConfig(height=3, width=4, char_polygons=[]).enable_debug is False


@pytest.mark.parametrize('config', [
    dict(gaussian_map_char_radius=0), dict(gaussian_map_char_radius=1025), dict(gaussian_map_char_radius=2.5),
    dict(gaussian_map_char_radius=True), dict(gaussian_map_distance_factor=0.0), dict(gaussian_map_distance_factor=1e-50),
    dict(gaussian_map_distance_factor=float('inf')), dict(gaussian_map_distance_factor=float('nan')),
    dict(gaussian_map_distance_factor=1e39), dict(gaussian_map_preserving_score_min=float('nan')),
    dict(gaussian_map_preserving_score_min=1e39), dict(weight_neutralized_score_map=-0.01),
    dict(weight_neutralized_score_map=1.01), dict(weight_neutralized_score_map=float(np.nextafter(1.0, 2.0))),
    dict(weight_neutralized_score_map=-5e-324), dict(weight_neutralized_score_map=float('nan')),
])
def test_refused_configs(config):
    from vkit_amd.engine.char_heatmap import char_heatmap_default_engine_executor_factory as F
    with pytest.raises(ValueError):
        F.create(config)


def test_refused_runs():
    """a quad without 4 points or with a non-finite point: ValueError before any launch (no GPU needed to see it)"""
    from vkit_amd.element import Polygon
    from vkit_amd.engine.char_heatmap import char_heatmap_default_engine_executor_factory as F
    ex = F.create()
    tri = Polygon.from_smooth_xy(np.array([(1, 1), (5, 1), (5, 5)], np.float64))
    nan = Polygon.from_smooth_xy(np.array([(1, 1), (5, np.nan), (5, 5), (1, 5)], np.float64))
    for polygons in ([tri], [nan]):
        with pytest.raises(ValueError):
            ex.run({'height': 10, 'width': 10, 'char_polygons': polygons})


def test_range_bound_at_the_weight_boundary():
    """DESIGN.md (char heatmap): score = f32(1 - w) * max + f32(w) * nscore <= f32(1 - w) + f32(w) <= 1 for max, nscore in
    [0, 1], so every accepted weight keeps the score in [0, 1].  Check the bound's premise on the accepted weights next to
    the boundary and on a dense sweep, and the score itself over values next to 1."""
    from vkit_amd.engine.char_heatmap.default import score_weights, weight_in_range
    rng = default_rng(5)
    near = [0.0, 5e-324, 1e-300, float(np.nextafter(0.0, 1.0)), float(np.float32(1e-45)), 0.4, 0.5,
            float(np.nextafter(1.0, 0.0)), 1.0 - 2 ** -24, 1.0 - 2 ** -25, 1.0 - 3 * 2 ** -26, 1.0]
    near += [float(np.nextafter(np.float32(v), np.float32(k))) for v in rng.uniform(0, 1, 200) for k in (0, 1)]
    weights = [float(w) for w in near + list(rng.uniform(0, 1, 20000)) + list(np.linspace(0, 1, 20001))]
    values = np.array([0.0, 1e-45, 0.5, 0.9, np.nextafter(np.float32(1), np.float32(0)), 1.0], np.float32)
    mx, ns = np.meshgrid(values, values)
    for w in weights:
        assert weight_in_range(w), w
        a, b = score_weights(w)
        assert a >= 0 and b >= 0 and np.float32(a + b) <= 1, w
        score = (1 - w) * mx + w * ns
        assert score.dtype == np.float32 and 0 <= score.min() and score.max() <= 1, w
    for w in (-1e-300, -0.0 - 1e-16, float(np.nextafter(1.0, 2.0)), 2.0, float('inf')):
        assert not weight_in_range(w), w


def test_bilinear_sample_stays_in_range():
    """the premise of the warp bound: the four float32 bilinear weights are exact and their partial sums too, so a sample of
    values in [0, 1] stays in [0, 1] (an all-ones template gives exactly 1 at every in-range sample)"""
    for fy in range(32):
        for fx in range(32):
            ax, ay = np.float32(fx) * np.float32(1 / 32), np.float32(fy) * np.float32(1 / 32)
            bx, by = np.float32(1) - ax, np.float32(1) - ay
            w = [by * bx, by * ax, ay * bx, ay * ax]
            assert np.float32(np.float32(w[0] + w[1]) + w[2]) + w[3] == np.float32(1)
            assert sum(float(v) for v in w) == 1.0


def test_oracle_fill_poly_equals_its_closed_form_on_char_quads():
    """the raster decides fillPoly membership by the closed form (outline + even-odd spans); the reference path of the
    golden is oracle.fill_poly: the two agree on char-like and degenerate quads"""
    import oracle as O
    rng = default_rng(11)
    quads = [np.array(q) for q in ([(0, 0), (0, 0), (0, 0), (0, 0)], [(0, 0), (8, 4), (16, 8), (24, 12)],
                                   [(0, 0), (26, 20), (26, 0), (0, 20)], [(0, 5), (5, 0), (10, 5), (5, 10)])]
    for _ in range(400):
        q = rng.integers(0, rng.integers(1, 40), (4, 2))
        quads.append(q)
    for q in quads:
        rel = q - q.min(axis=0)
        shape = (int(rel[:, 1].max()) + 1, int(rel[:, 0].max()) + 1)
        assert np.array_equal(O.fill_poly(shape, rel), O.fill_poly(shape, rel, closed_form=True)), q.tolist()
