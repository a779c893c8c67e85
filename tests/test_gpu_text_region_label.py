"""PageTextRegionLabelStep on the GPU (vkit_amd/pipeline/text_detection/page_text_region_label.py, csrc/region_label.hip):
the step against the reference's own runs (tests/golden/text_region_label.npz) on host and device pages, against the
restatement (tests/text_region_label_restate.py) on 1024² pages and seeded pages, the tie path with and without sklearn, the
inactive region, the launch and synchronisation budget and ABI refusals."""
import builtins
import os
import sys
import time

import numpy as np
import pytest
from numpy.random import default_rng

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import char_heatmap_restate as HR  # noqa: E402
import text_region_label_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = R.load_golden()
ERRORS = {'AssertionError': AssertionError, 'ValueError': ValueError}
PLANES = {'char_mask': 'page_char_mask', 'height': 'page_char_height_score_map',
          'gaussian': 'page_char_gaussian_score_map', 'box_mask': 'page_char_bounding_box_mask'}


def _run(quads, shape, active, rng, resident, num=1, factor=3):
    from vkit_amd import _native as N
    from vkit_amd.element import Image, Mask, Polygon
    from vkit_amd.pipeline.text_detection import (PageTextRegionLabelStepInput, PageTextRegionStepOutput,
                                                  page_text_region_label_step_factory as F)
    polygons = [Polygon.from_smooth_xy(q) for q in quads]
    image, mask = np.zeros(tuple(shape) + (3,), np.uint8), np.ascontiguousarray(active, np.uint8)
    if resident:
        ctx = N.default_ctx()
        image, mask = ctx.to_device(image), ctx.to_device(mask)
    src = PageTextRegionStepOutput(page_image=Image(mat=image), page_active_mask=Mask(mat=mask), page_char_polygons=polygons,
                                   page_text_region_polygons=polygons,
                                   page_char_polygon_text_region_polygon_indices=list(range(len(polygons))),
                                   shape_before_rotate=tuple(shape), rotate_angle=0, debug=None)
    step = F.create({'num_deviate_char_regression_labels': num, 'num_deviate_char_regression_labels_candiates_factor': factor})
    return step.run(PageTextRegionLabelStepInput(page_text_region_step_output=src), rng)


def _labels(out):
    return [(lb.char_idx, int(lb.tag.value == 'deviate'), lb.label_point_smooth_y, lb.label_point_smooth_x,
             lb.downsampled_label_point_y, lb.downsampled_label_point_x) for lb in out.page_char_regression_labels]


def _assert_equal(out, want_planes, want_labels, resident):
    from vkit_amd import _native as N
    for name, field in PLANES.items():
        element = getattr(out, field)
        assert isinstance(element.arr, N.DevArray) == resident, name
        assert element.mat.dtype == want_planes[name].dtype and element.mat.tobytes() == want_planes[name].tobytes(), name
    assert _labels(out) == want_labels


@pytest.mark.parametrize('resident', [False, True], ids=['host', 'device'])
@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_step_equals_the_reference(case, resident, caplog):
    rng = default_rng(case['seed'])
    args = (case['quads'], case['shape'], case['active'], rng, resident, case['num'], case['factor'])
    caplog.set_level('WARNING', logger='vkit_amd.pipeline.text_detection.page_text_region_label')
    if 'raises' in case:
        with pytest.raises(ERRORS[case['raises']]):
            _run(*args)
    else:
        out = _run(*args)
        _assert_equal(out, case, R.golden_labels(case), resident)
        assert [lb.valid for lb in out.page_char_regression_labels] == case['label_valid'].astype(bool).tolist()
        warned = [r for r in caplog.records if 'Cannot sample enough deviate labels' in r.getMessage()]
        assert len(warned) == case['warnings']
    assert R.rng_state(rng) == case['rng_state']


def _page(seed, shape=(1024, 1024), n=1000, active=True):
    rng = default_rng(seed)
    quads = HR.text_line_quads(rng, shape, n, height=(16, 28), step=(0.75, 1.05))
    act = np.ones(shape, np.uint8)
    if not active:
        act[: shape[0] // 3, shape[1] // 2:] = 0
    return quads, act


@pytest.mark.parametrize('seed,resident,num', [(0, True, 1), (1, False, 2), (2, True, 3)])
def test_large_pages_equal_the_restatement(seed, resident, num):
    quads, act = _page(seed, active=seed != 1)
    assert len(quads) >= 900
    want_warnings = []
    want = R.run(quads, (1024, 1024), act, default_rng(seed), num=num, warnings=want_warnings)
    rng = default_rng(seed)
    out = _run(quads, (1024, 1024), act, rng, resident, num=num)
    _assert_equal(out, want, want['labels'], resident)


def _grid_page(rows=25, cols=40, size=12, pitch=10):
    """a regular grid of overlapping axis-aligned chars: integer points half way between two centres lie inside both"""
    quads = []
    for r in range(rows):
        for c in range(cols):
            x0, y0 = 4 + c * pitch, 4 + r * pitch
            quads.append([(x0, y0), (x0 + size, y0), (x0 + size, y0 + size), (x0, y0 + size)])
    return np.asarray(quads, np.float64), (rows * pitch + size + 8, cols * pitch + size + 8)


def test_tie_path_with_sklearn():
    """a regular grid: many candidates tie between neighbouring centres; sklearn's tree answers them as the reference's"""
    from vkit_amd.pipeline.text_detection import page_text_region_label as M
    quads, shape = _grid_page()
    act = np.ones(shape, np.uint8)
    calls = []
    real = M._resolve_ties
    M._resolve_ties = lambda *a: calls.append(len(a[1])) or real(*a)
    try:
        out = _run(quads, shape, act, default_rng(5), True, num=3)
    finally:
        M._resolve_ties = real
    assert calls and calls[0] > 50
    want = R.run(quads, shape, act, default_rng(5), num=3)
    _assert_equal(out, want, want['labels'], True)


def test_tie_path_without_sklearn(monkeypatch, caplog):
    """sklearn not importable: the lowest centre index wins a tie, with one warning"""
    from vkit_amd.pipeline.text_detection.page_text_region_label import _resolve_ties
    real_import = builtins.__import__

    def no_sklearn(name, *args, **kwargs):
        if name.startswith('sklearn'):
            raise ImportError('no sklearn')
        return real_import(name, *args, **kwargs)

    monkeypatch.setattr(builtins, '__import__', no_sklearn)
    centres = np.array([(10, 10), (14, 10), (12, 14)], np.int32)
    points = np.array([(12, 10), (12, 10), (13, 12)], np.int32)      # ties 0-1, 0-1 and 1-2
    keep = _resolve_ties(centres, points, np.array([0, 1, 2]))
    assert keep.tolist() == [True, False, False]
    quads, shape = _grid_page(8, 10)
    caplog.set_level('WARNING')
    out = _run(quads, shape, np.ones(shape, np.uint8), default_rng(9), True, num=2)
    assert any('sklearn' in r.getMessage() for r in caplog.records)
    assert len(out.page_char_regression_labels) >= len(quads)


def test_inactive_region_is_zeroed():
    quads, act = _page(4, shape=(256, 320), n=150, active=False)
    out = _run(quads, (256, 320), act, default_rng(4), True)
    inactive = act == 0
    assert inactive.any() and (out.page_char_mask.mat[inactive] == 0).all()
    assert (out.page_char_height_score_map.mat[inactive] == 0).all()
    assert out.page_char_mask.mat[~inactive].any()


@pytest.mark.parametrize('num', [0, 1])
@pytest.mark.parametrize('n', [20, 1500])
def test_device_run_launches_and_syncs(n, num, monkeypatch):
    """a device-resident page: a bounded number of launches whatever the char count; one Context.sync with deviates, none
    without"""
    from vkit_amd import _native as N
    ctx = N.default_ctx()
    quads = HR.text_line_quads(default_rng(n), (1024, 1024), n, height=(12, 20))
    act = np.ones((1024, 1024), np.uint8)
    _run(quads, (1024, 1024), act, default_rng(0), True, num=num)      # warm the scratch slots
    ctx.sync()
    syncs = []
    real_sync = N.Context.sync
    monkeypatch.setattr(N.Context, 'sync', lambda self: syncs.append(1) or real_sync(self))
    ctx.set_timing(1)
    try:
        ctx.reset_timings()
        out = _run(quads, (1024, 1024), act, default_rng(0), True, num=num)
        calls_syncs = list(syncs)
        timings = ctx.timings()
    finally:
        ctx.set_timing(0)
    ours = {name: cnt for name, (_ms, cnt) in timings.items() if name.startswith('k_region_label')}
    assert ours == ({'k_region_label_planes': 1, 'k_region_label_deviate': 1} if num else {'k_region_label_planes': 1})
    assert sum(cnt for _ms, cnt in timings.values()) <= 12, timings
    assert calls_syncs == ([1] if num else [])
    assert isinstance(out.page_char_mask.arr, N.DevArray)


def test_abi_refusals_leave_canaries():
    from vkit_amd import _native as N
    L = N.lib()
    ctx = N.default_ctx()
    h, w = 40, 50
    active = ctx.to_device(np.zeros((h, w), np.uint8))
    cmask = ctx.to_device(np.full((h, w), 0xAB, np.uint8))
    height = ctx.to_device(np.full((h, w), 7.5, np.float32))
    bmask = ctx.to_device(np.full((h, w), 0xCD, np.uint8))
    boxes = np.array([[2, 10, 3, 20]], np.int32)

    def planes(bx=boxes, n=None, hh=h, ww=w, a=active, c=cmask, s=height, b=bmask):
        bx = np.ascontiguousarray(bx, np.int32)
        return L.vkx_region_label_planes_dev(ctx.handle, bx.ctypes.data if bx is not None else None,
                                             len(bx) if n is None else n, hh, ww, a.ptr if a is not None else None,
                                             c.ptr if c is not None else None, s.ptr if s is not None else None,
                                             b.ptr if b is not None else None)

    out = ctx.to_device(np.full(64 * 8, 0x5A, np.uint8))
    sq = np.array([[(10, 10), (20, 10), (20, 20), (10, 20)]], np.float64)
    centres = np.array([(15, 15)], np.int32)
    draws = np.array([[(1, 1), (5, 5), (9, 9)]], np.int32)

    def deviate(q=sq, c=centres, nc=None, n=1, d=draws, m=3, hh=h, ww=w, o=out):
        q, c, d = (np.ascontiguousarray(v) for v in (q, c, d))
        return L.vkx_region_label_deviate_dev(ctx.handle, q.ctypes.data, c.ctypes.data, len(c) if nc is None else nc, n,
                                              d.ctypes.data, m, hh, ww, o.ptr if o is not None else None)

    cases = {
        'planes: NULL active': lambda: planes(a=None),
        'planes: NULL box mask': lambda: planes(b=None),
        'planes: negative count': lambda: planes(n=-1),
        'planes: h 0': lambda: planes(hh=0),
        'planes: w 32769': lambda: planes(ww=32769),
        'planes: box below the page': lambda: planes(bx=[[2, 40, 3, 20]]),
        'planes: box up < 0': lambda: planes(bx=[[-1, 10, 3, 20]]),
        'planes: box left > right': lambda: planes(bx=[[2, 10, 21, 20]]),
        'planes: mask twice': lambda: planes(b=cmask),
        'planes: height over the box mask': lambda: planes(s=N.DevArray(ctx, bmask.ptr, (h, w), np.float32, 0)),
        'deviate: NULL out': lambda: deviate(o=None),
        'deviate: no centres': lambda: deviate(nc=0),
        'deviate: more chars than centres': lambda: deviate(n=2),
        'deviate: m 0': lambda: deviate(m=0),
        'deviate: m 4097': lambda: deviate(m=4097),
        'deviate: page 32769': lambda: deviate(hh=32769),
        'deviate: non-finite point': lambda: deviate(q=np.where(sq == 20, np.nan, sq)),
        'deviate: box of height 2': lambda: deviate(q=np.array([[(10, 10), (20, 10), (20, 11), (10, 11)]], np.float64)),
        'deviate: draw outside the box': lambda: deviate(d=np.array([[(1, 1), (5, 5), (10, 9)]], np.int32)),
        'deviate: draw 0': lambda: deviate(d=np.array([[(0, 1), (5, 5), (9, 9)]], np.int32)),
        'deviate: centre too far': lambda: deviate(c=np.array([(1 << 30, 0)], np.int32)),
    }
    for name, fn in cases.items():
        assert fn() == N.ERR_INVALID, name
    ctx.sync()
    for p, v in ((cmask, 0xAB), (height, np.float32(7.5)), (bmask, 0xCD), (out, 0x5A)):
        p.invalidate_host()
        assert (p.host() == v).all()
    # and valid calls write them
    assert planes() == 0 and deviate() == 0
    ctx.sync()
    for p in (cmask, height, bmask, out):
        p.invalidate_host()
    assert (cmask.host() == 0).all() and (height.host() == 0).all()
    assert bmask.host()[2:11, 3:21].all() and bmask.host().sum() == 9 * 18
    rec = out.host()[:3 * 32].view(N.REGION_LABEL_DEVIATE_DTYPE)
    assert (rec['status'] == 0).all() and rec['iy'].tolist() == [11, 15, 19] and rec['ix'].tolist() == [11, 15, 19]


def _planes_against_numpy(shape, boxes, active):
    """vkx_region_label_planes_dev on planes of ``shape`` that start from fixed patterns, against numpy"""
    from vkit_amd import _native as N
    ctx = N.default_ctx()
    ys, xs = np.indices(shape)
    cmask0 = ((ys + xs) % 3 != 0).astype(np.uint8)
    height0 = ((ys * 5 + xs) % 7 + 1).astype(np.float32)
    cmask, height, bmask = ctx.to_device(cmask0), ctx.to_device(height0), N.dev_full(shape, 0xCD, ctx=ctx)
    N.region_label_planes(boxes, ctx.to_device(active), cmask, height, bmask)
    want = np.zeros(shape, np.uint8)
    for up, down, left, right in boxes:
        want[up:down + 1, left:right + 1] = 1
    assert np.array_equal(bmask.host(), want)
    assert np.array_equal(cmask.host(), np.where(active == 0, 0, cmask0).astype(np.uint8))
    assert np.array_equal(height.host(), np.where(active == 0, 0, height0).astype(np.float32))


SMALL, WHOLE_TILE = (40, 50, 40, 50), (32, 63, 32, 63)
TILE_BOXES = [SMALL, WHOLE_TILE, (32, 63, 32, 62), (64, 69, 96, 99), (0, 69, 0, 99), SMALL]
TILE_BOX_LISTS = [[box] for box in TILE_BOXES[:5]] + [
    [SMALL, WHOLE_TILE, SMALL], [SMALL, (32, 63, 32, 62), SMALL], [SMALL, WHOLE_TILE, (32, 63, 32, 62), (64, 69, 96, 99), SMALL],
    [SMALL, (64, 69, 96, 99), (32, 63, 32, 62)], TILE_BOXES, []]


@pytest.mark.parametrize('backwards', [False, True], ids=['listed', 'reversed'])
@pytest.mark.parametrize('case', range(len(TILE_BOX_LISTS)))
def test_planes_at_the_tile_borders(case, backwards):
    """A 70 x 100 page (3 x 4 tiles of 32 x 32, the last row and column clipped): a box that is a whole tile, one a column short of
    it, the clipped corner tile covered whole, the whole page, and a small box listed before and after the box that makes its tile
    whole, in both orders; the active mask has a zero band across tile borders."""
    active = np.ones((70, 100), np.uint8)
    active[30:35, :] = 0
    active[:, 60:66] = 0
    boxes = TILE_BOX_LISTS[case][::-1] if backwards else TILE_BOX_LISTS[case]
    _planes_against_numpy((70, 100), np.array(boxes, np.int32).reshape(-1, 4), active)


def test_planes_refuse_too_many_box_tile_pairs():
    """One more row of 1024 (box, tile) pairs than the bound of 2^28: refused while the pairs are counted, nothing written; the same
    table cut to 8 boxes is a call like any other.  (No success case near the bound: it would stage a gigabyte.)"""
    from vkit_amd import _native as N
    ctx = N.default_ctx()
    h, w = 32, 32768
    n = (1 << 28) // 1024 + 1
    boxes = np.zeros((n, 4), np.int32)
    boxes[:, 3] = w - 1                                    # row 0 of every tile: no tile is covered whole
    active = ctx.to_device(np.zeros((h, w), np.uint8))
    cmask, bmask = N.dev_full((h, w), 0xAB, ctx=ctx), N.dev_full((h, w), 0xCD, ctx=ctx)
    height = ctx.to_device(np.full((h, w), 7.5, np.float32))
    rc = N.lib().vkx_region_label_planes_dev(ctx.handle, boxes.ctypes.data, n, h, w, active.ptr, cmask.ptr, height.ptr, bmask.ptr)
    assert rc == N.ERR_INVALID and 'too many (box, tile) pairs' in N.last_error()
    ctx.sync()
    for p in (cmask, bmask, height):
        p.invalidate_host()
    assert (cmask.host() == 0xAB).all() and (bmask.host() == 0xCD).all() and (height.host() == np.float32(7.5)).all()
    band = np.ones((h, w), np.uint8)
    band[:, 1000:1100] = 0
    _planes_against_numpy((h, w), boxes[:8], band)


def test_soak_seeded_pages():
    """seeded pages of varying size, char count, config, activity and placement: every one equals the restatement"""
    rng = default_rng(2027)
    t0 = time.time()
    pages = 0
    while time.time() - t0 < 20 or pages < 5:
        h, w = int(rng.integers(48, 360)), int(rng.integers(48, 360))
        n = int(rng.integers(1, 200))
        quads = HR.text_line_quads(rng, (h, w), n, height=(6, min(h, w) * 0.3 + 7), step=(0.6, 1.1), tilt=0.4, jitter=0.1)
        if len(quads) == 0:
            continue
        act = np.ones((h, w), np.uint8)
        act[int(rng.integers(0, h)):, int(rng.integers(0, w)):] = 0
        num, factor, seed = int(rng.integers(0, 4)), int(rng.integers(1, 4)), int(rng.integers(0, 1 << 30))
        resident = bool(rng.integers(0, 2))
        want_rng, got_rng = default_rng(seed), default_rng(seed)
        try:
            want = R.run(quads, (h, w), act, want_rng, num=num, factor=factor)
        except (AssertionError, ValueError) as e:
            with pytest.raises(type(e)):
                _run(quads, (h, w), act, got_rng, resident, num=num, factor=factor)
        else:
            out = _run(quads, (h, w), act, got_rng, resident, num=num, factor=factor)
            _assert_equal(out, want, want['labels'], resident)
        assert R.rng_state(got_rng) == R.rng_state(want_rng)
        pages += 1
        if pages >= 300:
            break
    assert time.time() - t0 < 120
