"""The default char-heatmap engine on the GPU (vkit_amd/engine/char_heatmap/, csrc/char_heatmap.hip): the engine against
the reference's own runs (tests/golden/char_heatmap.npz) on host and device planes, against the restatement
(tests/char_heatmap_restate.py) on text-line pages, the per-pixel fillPoly test against the oracle's rasters, order
independence, the self-clearing scratch, the launch and synchronisation budget, ABI refusals and a seeded soak."""
import os
import sys
import time

import numpy as np
import pytest
from numpy.random import default_rng

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import char_heatmap_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = R.load_golden()
ERRORS = {'AssertionError': AssertionError, 'IndexError': IndexError}


def _polygons(quads):
    from vkit_amd.element import Polygon
    return [Polygon.from_smooth_xy(q) for q in np.asarray(quads, np.float64).reshape(-1, 4, 2)]


def _executor(radius=25, factor=2.25, preserving=0.9, weight=0.4):
    from vkit_amd.engine.char_heatmap import char_heatmap_default_engine_executor_factory as F
    return F.create({'gaussian_map_char_radius': radius, 'gaussian_map_distance_factor': factor,
                     'gaussian_map_preserving_score_min': preserving, 'weight_neutralized_score_map': weight})


def _run(quads, shape, resident, debug=True, polygons=None, **config):
    from vkit_amd import _native as N
    run_config = {'height': shape[0], 'width': shape[1], 'enable_debug': debug,
                  'char_polygons': polygons if polygons is not None else _polygons(quads)}
    with N.resident(resident):
        return _executor(**config).run(run_config)


def _planes(out):
    planes = {'score': out.score_map.mat}
    if out.debug is not None:
        planes.update({name: getattr(out.debug, name).mat for name in R.DEBUG_NAMES})
    return planes


def _assert_bitwise(got, want, names):
    for name in names:
        assert got[name].dtype == want[name].dtype and got[name].tobytes() == want[name].tobytes(), name


@pytest.mark.parametrize('resident', [False, True], ids=['host', 'device'])
@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_engine_equals_the_reference(case, resident):
    from vkit_amd import _native as N
    shape = tuple(case['shape'])
    if 'raises' in case:
        with pytest.raises(ERRORS[case['raises']]):
            _run(case['quads'], shape, resident, debug=case['debug'], **R.config_of(case))
        return
    out = _run(case['quads'], shape, resident, debug=case['debug'], **R.config_of(case))
    assert isinstance(out.score_map.arr, N.DevArray) == resident
    assert out.score_map.is_prob and (out.debug is not None) == case['debug']
    _assert_bitwise(_planes(out), case, ('score',) + (R.DEBUG_NAMES if case['debug'] else ()))


def test_polygon_soup_input():
    from vkit_amd.element import PolygonSoup
    case = next(c for c in CASES if c['name'] == 'text-lines-0.8-axis')
    q = case['quads']
    soup = PolygonSoup(np.ascontiguousarray(q.reshape(-1, 2)), np.arange(0, 4 * len(q) + 1, 4, dtype=np.int64))
    out = _run(None, tuple(case['shape']), True, polygons=soup, **R.config_of(case))
    _assert_bitwise(_planes(out), case, ('score',) + R.DEBUG_NAMES)


@pytest.mark.parametrize('seed', [0, 1])
def test_text_line_pages_equal_the_restatement(seed):
    rng = default_rng(100 + seed)
    quads = R.text_line_quads(rng, (1024, 1024), 1000, step=(0.75, 1.0))
    assert len(quads) == 1000
    want = R.run(quads, (1024, 1024))
    assert want['neutralized_mask'].any() and want['char_overlapped_mask'].any()
    _assert_bitwise(_planes(_run(quads, (1024, 1024), True)), want, ('score',) + R.DEBUG_NAMES)


def test_large_chars_on_a_non_square_page():
    rng = default_rng(7)
    shape = (1536, 2048)
    quads = R.text_line_quads(rng, shape, 300, height=(60, 180), step=(0.7, 1.0), tilt=0.3, jitter=0.12)
    want = R.run(quads, shape, radius=40, factor=3.5, preserving=0.8, weight=0.25)
    got = _planes(_run(quads, shape, False, radius=40, factor=3.5, preserving=0.8, weight=0.25))
    _assert_bitwise(got, want, ('score',) + R.DEBUG_NAMES)


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_overlap_mask_of_doubled_quads_is_the_union_of_fill_poly(seed):
    """every quad twice: char_overlapped_mask is exactly the union of the oracle's fillPoly rasters -- the raster's
    per-pixel membership test, pinned directly (degenerate, tiny and steep quads included)"""
    import oracle as O
    rng = default_rng(300 + seed)
    shape = (200, 260)
    quads = R.text_line_quads(rng, shape, 120, height=(3, 40), tilt=0.8, jitter=0.3)
    quads = np.concatenate([quads, np.full((1, 4, 2), 50.0), [[(5, 5), (60, 30), (60, 5), (5, 30)]],
                            [[(100, 100), (150, 110), (200, 120), (250, 130)]], [[(20, 40), (25, 190), (30, 60), (22, 100)]]])
    want = np.zeros(shape, np.uint8)
    for q in quads:
        rel, (up, down, left, right) = R.char_geometry(q)
        want[up:down + 1, left:right + 1] |= O.fill_poly((down - up + 1, right - left + 1), rel.astype(np.int32))
    out = _run(np.concatenate([quads, quads[::-1]]), shape, True)
    assert np.array_equal(out.debug.char_overlapped_mask.mat, want)


@pytest.mark.parametrize('bw,bh', [(32, 8), (33, 9)])
def test_boxes_at_the_tile_borders(bw, bh):
    """axis-aligned chars whose boxes are exactly one 32 x 8 tile, and 33 x 9: one pixel into a second tile row and column; two
    overlapping chars and one in the page's last rows and columns, against the restatement"""
    shape = (40, 100)
    quads = np.array([[(x, y), (x + bw - 1, y), (x + bw - 1, y + bh - 1), (x, y + bh - 1)]
                      for x, y in ((5, 3), (20, 7), (shape[1] - bw, shape[0] - bh))], np.float64)
    assert all(R.char_geometry(q)[1] == (int(q[0, 1]), int(q[0, 1]) + bh - 1, int(q[0, 0]), int(q[0, 0]) + bw - 1) for q in quads)
    want = R.run(quads, shape)
    assert want['char_overlapped_mask'].any()
    _assert_bitwise(_planes(_run(quads, shape, True)), want, ('score',) + R.DEBUG_NAMES)


def test_permuted_chars_give_identical_planes():
    rng = default_rng(9)
    quads = R.text_line_quads(rng, (512, 640), 500, step=(0.6, 0.9))
    a = _planes(_run(quads, (512, 640), True))
    b = _planes(_run(quads[rng.permutation(len(quads))], (512, 640), True))
    _assert_bitwise(b, a, ('score',) + R.DEBUG_NAMES)


def test_consecutive_calls_clear_the_scratch():
    """two calls in a row on different pages (and page sizes) each equal a fresh run of the restatement"""
    rng = default_rng(13)
    pages = [((300, 400), R.text_line_quads(rng, (300, 400), 200, step=(0.6, 0.9))),
             ((300, 400), R.text_line_quads(rng, (300, 400), 150, step=(0.7, 1.0))),
             ((200, 500), R.text_line_quads(rng, (200, 500), 120)),
             ((300, 400), np.zeros((0, 4, 2)))]
    outs = [_planes(_run(q, shape, True)) for shape, q in pages]
    for (shape, q), got in zip(pages, outs):
        _assert_bitwise(got, R.run(q, shape), ('score',) + R.DEBUG_NAMES)


def test_refused_call_leaves_the_next_one_clean():
    bad = next(c for c in CASES if c.get('raises') == 'IndexError')
    good = next(c for c in CASES if c['name'] == 'duplicated')
    with pytest.raises(IndexError):
        _run(bad['quads'], tuple(bad['shape']), True)
    out = _run(good['quads'], tuple(good['shape']), True)
    _assert_bitwise(_planes(out), good, ('score',) + R.DEBUG_NAMES)


@pytest.mark.parametrize('n', [10, 2000])
def test_device_run_launches_and_syncs(n, monkeypatch):
    """a device-resident page: at most 3 k_char_heatmap_* launches whatever the char count, and no Context.sync"""
    from vkit_amd import _native as N
    ctx = N.default_ctx()
    quads = R.text_line_quads(default_rng(n), (1024, 1024), n, height=(12, 20))
    assert len(quads) == n
    _run(quads, (1024, 1024), True)       # warm the scratch slots
    ctx.sync()
    syncs = []
    real_sync = N.Context.sync
    monkeypatch.setattr(N.Context, 'sync', lambda self: syncs.append(1) or real_sync(self))
    ctx.set_timing(1)
    try:
        ctx.reset_timings()
        out = _run(quads, (1024, 1024), True, debug=False)
        calls_syncs = list(syncs)
        timings = ctx.timings()
    finally:
        ctx.set_timing(0)
    ours = {name: cnt for name, (_ms, cnt) in timings.items() if name.startswith('k_char_heatmap')}
    assert set(ours) == {'k_char_heatmap_setup', 'k_char_heatmap_raster', 'k_char_heatmap_resolve'}, timings
    assert sum(ours.values()) == 3, timings
    assert calls_syncs == []
    assert isinstance(out.score_map.arr, N.DevArray)


def test_abi_refusals_leave_canaries():
    import ctypes
    from vkit_amd import _native as N
    L = N.lib()
    ctx = N.default_ctx()
    h, w = 40, 50
    score = ctx.to_device(np.full((h, w), 7.5, np.float32))
    f32 = [ctx.to_device(np.full((h, w), 7.5, np.float32)) for _ in range(4)]
    u8 = [ctx.to_device(np.full((h, w), 0xAB, np.uint8)) for _ in range(2)]
    gauss = np.ones((51, 51), np.float32)
    sq = np.array([[(10, 10), (20, 10), (20, 20), (10, 20)]], np.float64)

    def config(radius=25, tmpl=gauss):
        c = N.VkxCharHeatmapConfig()
        c.radius, c.template_host = radius, tmpl.ctypes.data if tmpl is not None else None
        c.preserving_score_min, c.weight_max, c.weight_neutralized = 0.9, 0.6, 0.4
        return c

    def debug(planes=None):
        p = planes or [f32[0], f32[1], u8[0], f32[2], u8[1], f32[3]]
        return N.VkxCharHeatmapDebug(*[x.ptr if x is not None else None for x in p])

    def call(cfg=None, quads=sq, n=None, hh=h, ww=w, out=score, dbg=None):
        quads = np.ascontiguousarray(quads, np.float64)
        return L.vkx_char_heatmap_fresh_dev(ctx.handle, ctypes.byref(cfg or config()) if cfg is not False else None,
                                            quads.ctypes.data, len(quads) if n is None else n, hh, ww,
                                            out.ptr if out is not None else None, ctypes.byref(dbg) if dbg else None)

    cases = {
        'NULL config': lambda: call(cfg=False),
        'NULL score': lambda: call(out=None),
        'NULL template': lambda: call(cfg=config(tmpl=None)),
        'radius 0': lambda: call(cfg=config(radius=0)),
        'radius 1025': lambda: call(cfg=config(radius=1025)),
        'negative n': lambda: call(n=-1),
        'n 2^24': lambda: call(n=1 << 24),
        'h 0': lambda: call(hh=0),
        'w too large': lambda: call(ww=1 << 24),
        'pixels >= 2^31': lambda: call(hh=1 << 16, ww=1 << 15),
        'non-finite point': lambda: call(quads=np.where(sq == 20, np.inf, sq)),
        'nan point': lambda: call(quads=np.where(sq == 20, np.nan, sq)),
        'box below the page': lambda: call(quads=sq + (0, 25)),
        'box left of the page': lambda: call(quads=sq - (11, 0)),
        'debug with a NULL plane': lambda: call(dbg=debug([f32[0], None, u8[0], f32[2], u8[1], f32[3]])),
        'score twice': lambda: call(dbg=debug([score, f32[1], u8[0], f32[2], u8[1], f32[3]])),
        'mask inside a float plane': lambda: call(dbg=debug([f32[0], f32[1], N.DevArray(ctx, f32[2].ptr + 8, (h, w), np.uint8, 0),
                                                            f32[2], u8[1], f32[3]])),
    }
    for name, fn in cases.items():
        assert fn() == N.ERR_INVALID, name
    ctx.sync()
    for p in [score] + f32:
        p.invalidate_host()
        assert (p.host() == np.float32(7.5)).all()
    for p in u8:
        p.invalidate_host()
        assert (p.host() == 0xAB).all()
    # and a valid call on the same planes writes them
    assert call(dbg=debug()) == 0
    score.invalidate_host()
    assert score.host()[15, 15] == np.float32(1.0) and score.host()[0, 0] == 0


def test_soak_seeded_pages():
    """seeded pages of varying size, char count, config and geometry: every one equals the restatement, bounded time"""
    rng = default_rng(2026)
    t0 = time.time()
    pages = 0
    while time.time() - t0 < 20 or pages < 5:
        h, w = int(rng.integers(32, 400)), int(rng.integers(32, 400))
        n = int(rng.integers(0, 300))
        quads = R.text_line_quads(rng, (h, w), n, height=(2, min(h, w) * 0.4 + 3), step=(0.5, 1.1), tilt=0.5, jitter=0.2)
        config = dict(radius=int(rng.choice([3, 12, 25, 40])), factor=float(rng.choice([0.7, 2.25, 3.5])),
                      preserving=float(rng.choice([0.5, 0.9, 0.95])), weight=float(rng.choice([0.0, 0.25, 0.4, 1.0])))
        resident = bool(rng.integers(0, 2))
        want = R.run(quads, (h, w), **config)
        got = _planes(_run(quads, (h, w), resident, **config))
        _assert_bitwise(got, want, ('score',) + R.DEBUG_NAMES)
        pages += 1
        if pages >= 1000:
            break
    assert time.time() - t0 < 120
