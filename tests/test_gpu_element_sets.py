"""The element set operations on the GPU (Mask.from_polygons / from_masks / from_score_maps and the fill_by_* families of Image,
Mask and ScoreMap in vkit_amd/element, csrc/element_sets.hip): the public methods against the reference's own runs
(tests/golden/element_sets.npz) on host and device-resident elements, a 200-polygon list against the numpy restatement
(tests/element_sets_restate.py), repeated runs and a cold scratch (order independence), a fill issued inside an open
deferred_fill, the launch and synchronisation budgets, the raw entry points on offset, padded and windowed planes between
canaries, and the ABI refusals.  Every comparison is exact (float32 as uint32 patterns)."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import element_sets_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'element_sets.npz')
FROM_CASES, FILL_CASES = R.from_cases(), R.fill_cases()
INVALID = -1


@pytest.fixture(scope='module')
def golden():
    data = np.load(GOLDEN)
    index = json.loads(str(data['index']))

    def get(ref):
        at, shape, dtype = ref
        return data[dtype][at:at + int(np.prod(shape))].reshape(shape)
    return ({e['name']: get(e['out']) for e in index['from_cases']}, {e['name']: get(e['out']) for e in index['fill_cases']})


def same(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
    assert got.tobytes() == want.tobytes(), int((got.view(np.uint8) != want.view(np.uint8)).sum())


def putter(resident):
    from vkit_amd import _native as N
    return (lambda a: N.default_ctx().to_device(np.ascontiguousarray(a))) if resident else None


def run_box(E, case):
    up, down, left, right = case['attached']
    return E.Box(up=up, down=down, left=left, right=right)


# ---- the constructors ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('resident', [False, True])
@pytest.mark.parametrize('kind', [R.BOXES, R.POLYGONS, R.MASKS, R.SCORE_MAPS])
def test_constructors_against_the_golden(kind, resident, golden):
    import vkit_amd.element as E
    from vkit_amd import _native as N
    want_all, _ = golden
    for case in (c for c in FROM_CASES if c['kind'] == kind):
        with N.resident(resident):
            runs = [R.run_from(E, case, putter(resident)) for _ in range(3)]
        for mask in runs:
            if kind != R.BOXES:        # (Mask.from_boxes is the host loop it was)
                assert isinstance(mask.arr, N.DevArray) == resident, case['name']
            attached = case['attached']
            assert (mask.box and (mask.box.up, mask.box.down, mask.box.left, mask.box.right)) == (attached and tuple(attached))
            same(mask.mat, want_all[case['name']])
            same(mask.mat, R.restate_from(case))
        if kind != R.BOXES:
            # the same list on a context whose scratch this list has not touched (a fresh context a case: cold planes, cold tables)
            from vkit_amd.element import _sets
            cold = N.Context(0)
            try:
                elements = R.build_elements(E, kind, case['elements'])
                where = run_box(E, case) if case['attached'] else case['shape']
                shape, attached_box = _sets.unpack_shape_or_box(where)
                got = N.set_mask(_sets.set_entries(kind, elements, attached_box), shape, R.mode_of(E, case['mode']), ctx=cold)
                same(N.host_array(got), want_all[case['name']])
            finally:
                cold.close()


@pytest.mark.parametrize('resident', [False, True])
def test_two_hundred_quads_warm_cold_and_reversed(resident):
    """the 200-polygon list on 256 x 256 in every mode: three runs, the list reversed (a set does not know its order) and a
    context whose scratch has never been used give the same plane as the restatement"""
    import vkit_amd.element as E
    from vkit_amd import _native as N
    polygons, shape = R.big_case()
    cold = N.Context(0)
    try:
        for mode in R.MODES:
            want = R.set_mask(R.POLYGONS, polygons, shape, mode)
            assert want.any()
            case = dict(kind=R.POLYGONS, elements=polygons, attached=None, shape=shape, mode=mode)
            with N.resident(resident):
                for _ in range(3):
                    mask = R.run_from(E, case)
                    assert isinstance(mask.arr, N.DevArray) == resident
                    same(mask.mat, want)
                same(R.run_from(E, dict(case, elements=polygons[::-1])).mat, want)
            same(N.host_array(N.set_mask(polygons, shape, E.ElementSetOperationMode(mode), ctx=cold)), want)
            got, windows = N.set_mask(polygons, shape, E.ElementSetOperationMode(mode), want_windows=True, ctx=cold)
            same(N.host_array(got), want)
            for polygon, window in zip(polygons, windows):
                same(N.host_array(window), R.own_raster(R.POLYGONS, polygon, shape)[1].astype(np.uint8))
    finally:
        cold.close()


# ---- the fills -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('resident', [False, True])
@pytest.mark.parametrize('dest', list(R.DESTS))
def test_fills_against_the_golden(dest, resident, golden):
    import vkit_amd.element as E
    from vkit_amd import _native as N
    _, want_all = golden
    seen = 0
    for case in (c for c in FILL_CASES if c['dest'] == dest):
        want = want_all[case['name']]
        for _ in range(3):
            out = R.run_fill(E, case, putter(resident))
            assert out.on_device == resident and isinstance(out.arr, N.DevArray) == resident, case['name']
            got = out.mat
            assert got.tobytes() == want.tobytes(), (case['name'], int((got != want).sum()))
        seen += 1
    assert seen >= 13


@pytest.mark.parametrize('resident', [False, True])
def test_fill_inside_an_open_deferred_fill(resident, golden):
    """the list joins the composite that is open on its destination: nothing is written before the block exits, and the layer
    recorded before it lies under the list's"""
    import vkit_amd.element as E
    from vkit_amd import _native as N
    from vkit_amd.element.opt import deferred_fill
    for name in ('fill_image3_polygons_union_mixed', 'fill_image3_polygons_distinct_mixed', 'fill_image3_masks_intersect_mixed'):
        case = next(c for c in FILL_CASES if c['name'] == name)
        first = E.Box(up=2, down=30, left=3, right=44)
        base = case['plane'].copy()
        base[2:31, 3:45] = (9, 8, 7)
        want = R.restate_fill(dict(case, plane=base))
        calls = []
        real = N.fill
        original = case['plane'].copy()
        dest = R.build_dest(E, case, putter(resident))
        try:
            N.fill = lambda *a, **k: calls.append(1) or real(*a, **k)
            with deferred_fill(dest.arr):
                first.fill_image(dest, (9, 8, 7))
                _fill_existing(E, case, dest, putter(resident))
                assert calls == []
                if not resident:
                    same(dest.arr, original)          # nothing is written yet
        finally:
            N.fill = real
        assert calls == [1]
        same(dest.mat, want)


def _fill_existing(E, case, dest, put):
    """run_fill's mixed form on a destination that exists already"""
    kind = case['kind']
    elements = R.build_elements(E, kind, case['elements'], put)
    values = [R.build_value(E, case, spec) for spec in case['values']]
    shape = case['plane'].shape[:2]
    tuples = [(e, v, R.alpha_of(case, i, R.box_of(kind, raw, shape), False))
              for i, (e, v, raw) in enumerate(zip(elements, values, case['elements']))]
    getattr(dest, f'fill_by_{R.SINGULAR[kind]}_value_tuples')(tuples, mode=R.mode_of(E, case['mode']))


def test_setitem_getitem_and_extract_score_map():
    import vkit_amd.element as E
    rng = np.random.default_rng(3)
    plane = rng.random(R.SHAPE, dtype=np.float32)
    polygon = E.Polygon.from_xy_pairs(R.CONCAVE)
    box, raster = R.own_raster(R.POLYGONS, np.array(R.CONCAVE, np.int32), R.SHAPE)
    score_map = E.ScoreMap(mat=plane.copy())
    got = score_map[polygon]
    want = plane[box[0]:box[1] + 1, box[2]:box[3] + 1].copy()
    want[~raster] = 0.0
    same(got.mat, want)
    assert got.box is None          # (extracted from a score map without a box: none is attached, as in the reference)
    same(E.Box(up=3, down=9, left=4, right=20).extract_score_map(score_map).mat, plane[3:10, 4:21])
    score_map[polygon] = E.ScoreMapSetItemConfig(value=0.75, keep_max_value=True)
    want = plane.copy()
    window = want[box[0]:box[1] + 1, box[2]:box[3] + 1]
    window[raster] = np.maximum(window[raster], np.float32(0.75))
    same(score_map.mat, want)
    mask = E.Mask(mat=np.zeros(R.SHAPE, np.uint8))
    mask[polygon] = 1
    mask[E.Box(up=0, down=3, left=0, right=3)] = E.MaskSetItemConfig(value=1)
    want = np.zeros(R.SHAPE, np.uint8)
    want[box[0]:box[1] + 1, box[2]:box[3] + 1][raster] = 1
    want[:4, :4] = 1
    same(mask.mat, want)
    same(mask[polygon].mat, raster.astype(np.uint8))
    same(mask[E.Box(up=0, down=5, left=0, right=5)].mat, want[:6, :6])


# ---- launches --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [10, 200])
@pytest.mark.parametrize('target', ['mask_distinct', 'image_union_half'])
def test_device_run_launches_and_syncs(n, target, monkeypatch):
    """a device-resident destination: at most 4 k_set_* launches whatever the polygon count, exactly one composite launch, no
    Context.sync, and the result stays on the device"""
    import vkit_amd.element as E
    from vkit_amd import _native as N
    ctx = N.default_ctx()
    polygons, shape = R.big_case(n)
    elements = R.build_elements(E, R.POLYGONS, polygons)

    def run():
        if target == 'mask_distinct':
            dest = E.Mask(mat=N.dev_zeros(shape, np.uint8, ctx))
            dest.fill_by_polygons(elements, mode=E.ElementSetOperationMode.DISTINCT)
        else:
            dest = E.Image(mat=N.dev_full(shape + (3,), 200, np.uint8, ctx))
            dest.fill_by_polygons(elements, (10, 20, 30), alpha=0.5)
        return dest

    run()       # warm the scratch slots
    ctx.sync()
    syncs = []
    real_sync = N.Context.sync
    monkeypatch.setattr(N.Context, 'sync', lambda self: syncs.append(1) or real_sync(self))
    ctx.set_timing(1)
    try:
        ctx.reset_timings()
        dest = run()
        calls_syncs = list(syncs)
        timings = ctx.timings()
    finally:
        ctx.set_timing(0)
    ours = {name: cnt for name, (_ms, cnt) in timings.items() if name.startswith('k_set_')}
    assert set(ours) <= {'k_set_outline', 'k_set_spans', 'k_set_planes', 'k_set_resolve'} and 1 <= sum(ours.values()) <= 4, timings
    composite = {name: cnt for name, (_ms, cnt) in timings.items() if name.startswith(('k_fill', 'k_composite'))}
    assert sum(composite.values()) == 1, timings
    assert calls_syncs == []
    assert isinstance(dest.arr, N.DevArray)
    # and it is the right plane
    if target == 'mask_distinct':
        same(dest.mat, R.set_mask(R.POLYGONS, polygons, shape, 'distinct'))
    else:
        case = dict(plane=np.full(shape + (3,), 200, np.uint8), kind=R.POLYGONS, elements=polygons, mode='union', keep=None,
                    values=[('tuple', (10, 20, 30))] * n, alphas='half', unique=True, dest='image3', seed=0)
        same(dest.mat, R.restate_fill(case))


# ---- the raw entry points --------------------------------------------------------------------------------------------------
def _raw_case():
    """boxes, polygons, a mask and a score map in one list on a 37 x 53 plane"""
    rng = np.random.default_rng(5)
    h, w = 37, 53
    mask = (R.blocky(rng, (11, 17), 3, 0.5)).astype(np.uint8) * np.uint8(200)
    score = rng.random((9, 21), dtype=np.float32) * 2 - 1
    elements = [(R.BOXES, (3, 20, 4, 30)), (R.POLYGONS, np.array([(2, 2), (50, 4), (40, 35), (10, 30)], np.int32)),
                (R.MASKS, (mask, (20, 30, 30, 46))), (R.SCORE_MAPS, (score, (0, 8, 10, 30))), (R.BOXES, (36, 36, 52, 52)),
                (R.POLYGONS, np.array([(2, 2), (50, 4), (40, 35), (10, 30)], np.int32))]
    return h, w, elements


def _raw_want(h, w, elements, mode, gated):
    count = np.zeros((h, w), np.int32)
    rasters = []
    for kind, element in elements:
        box, raster = R.own_raster(kind, element, (h, w))
        count[box[0]:box[1] + 1, box[2]:box[3] + 1][raster] += 1
        rasters.append((box, raster))
    dst = {0: count > 0, 1: count == 1, 2: count > 1}[mode].astype(np.uint8)
    windows = [(raster & (dst[b[0]:b[1] + 1, b[2]:b[3] + 1] > 0) if gated else raster).astype(np.uint8) for b, raster in rasters]
    return dst, windows


def _raw_records(N, elements, plane_ptrs, plane_steps, pad=7):
    recs = np.zeros(len(elements), N.SET_ELEM_DTYPE)
    pts, off = [], 0
    for i, (kind, element) in enumerate(elements):
        up, down, left, right = R.box_of(kind, element, None)
        rec = recs[i]
        rec['kind'] = {R.BOXES: N.SET_BOX, R.POLYGONS: N.SET_POLYGON, R.MASKS: N.SET_MASK_U8, R.SCORE_MAPS: N.SET_SCORE_F32}[kind]
        rec['up'], rec['left'], rec['h'], rec['w'] = up, left, down - up + 1, right - left + 1
        if kind == R.POLYGONS:
            rec['pts_off'], rec['pts_cnt'] = sum(len(p) for p in pts), len(element)
            pts.append(element)
        if i in plane_ptrs:
            rec['plane'], rec['plane_step'] = plane_ptrs[i], plane_steps[i]
        rec['window_off'] = off
        off += (down - up + 1) * (right - left + 1) + pad        # (odd offsets: the windows need no alignment)
    return recs, np.ascontiguousarray(np.concatenate(pts), np.int32), off


@pytest.mark.parametrize('gated', [False, True])
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_raw_dev_call_on_offset_padded_and_windowed_planes(mode, gated):
    from ctypes import c_void_p
    from vkit_amd import _native as N
    ctx, L = N.default_ctx(), N.lib()
    h, w, elements = _raw_case()
    dst_step, dst_at = w + 13, 259
    arena_host = np.full(1 << 16, 0xAB, np.uint8)
    # the mask plane at an odd offset with a padded step, the score plane at a float offset with a padded step
    mask, score = elements[2][1][0], elements[3][1][0]
    mask_at, mask_step = 8193, mask.shape[1] + 5
    score_at, score_step = 12288 + 4, (score.shape[1] + 3) * 4
    for r in range(mask.shape[0]):
        arena_host[mask_at + r * mask_step:mask_at + r * mask_step + mask.shape[1]] = mask[r]
    for r in range(score.shape[0]):
        arena_host[score_at + r * score_step:score_at + r * score_step + score.shape[1] * 4] = score[r].view(np.uint8)
    before = arena_host.copy()
    arena = ctx.to_device(arena_host)
    recs, pts, window_bytes = _raw_records(N, elements, {2: arena.ptr + mask_at, 3: arena.ptr + score_at}, {2: mask_step, 3: score_step})
    win_at = 20481
    rc = L.vkx_set_mask_dev(ctx.handle, recs.ctypes.data, len(recs), pts.ctypes.data, len(pts), mode | (N.SET_WINDOWS_GATED if gated else 0),
                            h, w, c_void_p(arena.ptr + dst_at), dst_step, c_void_p(arena.ptr + win_at), window_bytes)
    assert rc == 0, N.last_error()
    arena.invalidate_host()
    got = np.array(arena.host())
    want_dst, want_windows = _raw_want(h, w, elements, mode, gated)
    expect = before.copy()
    for r in range(h):
        expect[dst_at + r * dst_step:dst_at + r * dst_step + w] = want_dst[r]
    first_poly = min(int(r['window_off']) for r in recs if r['kind'] == N.SET_POLYGON)
    last_poly = max(int(r['window_off']) + int(r['h']) * int(r['w']) for r in recs if r['kind'] == N.SET_POLYGON)
    expect[win_at + first_poly:win_at + last_poly] = 0          # (vkx.h: zeroed between the first and the last polygon window)
    for i in range(len(recs)):          # (every window is written whole, the ones inside the zeroed range after the zeroing)
        at = win_at + int(recs[i]['window_off'])
        expect[at:at + want_windows[i].size] = want_windows[i].reshape(-1)
    assert got.tobytes() == expect.tobytes(), np.flatnonzero(got != expect)[:8]
    # the host form on host planes with the same steps
    host_dst = np.full((h, dst_step), 0xCD, np.uint8)
    host_windows = np.full(window_bytes + 32, 0xCD, np.uint8)
    host_mask = np.full((mask.shape[0], mask_step), 0xEE, np.uint8)
    host_mask[:, :mask.shape[1]] = mask
    host_score = np.full((score.shape[0], score_step // 4), -3.0, np.float32)
    host_score[:, :score.shape[1]] = score
    recs2, _, _ = _raw_records(N, elements, {2: host_mask.ctypes.data, 3: host_score.ctypes.data}, {2: mask_step, 3: score_step})
    rc = L.vkx_set_mask(ctx.handle, recs2.ctypes.data, len(recs2), pts.ctypes.data, len(pts), mode | (N.SET_WINDOWS_GATED if gated else 0),
                        h, w, host_dst.ctypes.data, dst_step, host_windows.ctypes.data, window_bytes)
    assert rc == 0, N.last_error()
    same(host_dst[:, :w], want_dst)
    assert (host_dst[:, w:] == 0xCD).all() and (host_windows[window_bytes:] == 0xCD).all()
    for i, rec in enumerate(recs2):
        at = int(rec['window_off'])
        same(host_windows[at:at + want_windows[i].size].reshape(want_windows[i].shape), want_windows[i])


def test_abi_refusals_leave_canaries():
    """every refusal of include/vkx.h is VKX_ERR_INVALID with nothing launched and the destination untouched; a clean call on the
    same context afterwards still matches"""
    from ctypes import c_void_p
    from vkit_amd import _native as N
    ctx, L = N.default_ctx(), N.lib()
    h, w, elements = _raw_case()
    mask, score = elements[2][1][0], elements[3][1][0]
    d_mask, d_score = ctx.to_device(mask), ctx.to_device(score)
    dst = ctx.to_device(np.full((h, w), 0xAB, np.uint8))
    recs, pts, window_bytes = _raw_records(N, elements, {2: d_mask.ptr, 3: d_score.ptr}, {2: mask.shape[1], 3: score.shape[1] * 4})
    windows = ctx.to_device(np.full(window_bytes, 0xCD, np.uint8))

    def call(r=recs, n=None, p=pts, n_pts=None, mode=1, hh=h, ww=w, d=dst.ptr, step=w, win=windows.ptr, nbytes=window_bytes):
        return L.vkx_set_mask_dev(ctx.handle, r.ctypes.data if r is not None else None, len(recs) if n is None else n,
                                  p.ctypes.data if p is not None else None, len(pts) if n_pts is None else n_pts, mode, hh, ww,
                                  c_void_p(d) if d else None, step, c_void_p(win) if win else None, nbytes)

    def edited(k=0, **fields):
        r = recs.copy()
        for name, value in fields.items():
            r[name][k] = value
        return r

    def moved(index, xy):
        q = pts.copy()
        q[index] = xy
        return q

    ctx.set_timing(1)
    try:
        ctx.reset_timings()
        refused = [
            call(n=-1), call(n=65537), call(r=None), call(d=0), call(p=None),                          # the count, NULL pointers
            call(mode=3), call(mode=-1), call(r=edited(kind=4)), call(r=edited(kind=-1)),              # unknown mode, unknown kind
            call(hh=0), call(ww=32768),                                                                 # the plane's sides
            call(r=edited(up=h - 17)), call(r=edited(left=-1)), call(r=edited(k=4, left=w)), call(r=edited(h=0)),   # a window outside h x w
            call(r=edited(k=2, w=w)),
            call(p=moved(0, (1, 2))), call(p=moved(2, (40, 36))),                                       # a vertex outside its window
            call(r=edited(k=1, pts_cnt=0)), call(r=edited(k=1, pts_off=-1)), call(r=edited(k=5, pts_cnt=5)), call(n_pts=7),
            call(r=edited(k=2, plane_step=mask.shape[1] - 1)), call(r=edited(k=2, plane_step=-mask.shape[1])),   # plane_step
            call(r=edited(k=3, plane_step=score.shape[1] * 4 - 1)),
            call(step=w - 1), call(step=-w),                                                            # dst_step
            call(nbytes=window_bytes - 8), call(r=edited(k=0, window_off=-1)),                          # window_bytes too small
            call(r=edited(k=2, plane=0)), call(r=edited(k=3, plane=0)),                                 # a NULL plane
            call(r=edited(k=2, plane=dst.ptr)), call(win=dst.ptr),                                      # overlapping planes
        ]
        assert refused == [INVALID] * len(refused), refused
        assert ctx.timings() == {}                     # nothing was launched
    finally:
        ctx.set_timing(0)
    dst.invalidate_host()
    windows.invalidate_host()
    assert (dst.host() == 0xAB).all() and (windows.host() == 0xCD).all()
    assert call() == 0
    dst.invalidate_host()
    same(dst.host(), _raw_want(h, w, elements, 1, False)[0])
    # an empty list: no launch, the h x w window zeroed and nothing else
    padded = ctx.to_device(np.full((h, w + 5), 0xAB, np.uint8))
    ctx.set_timing(1)
    try:
        ctx.reset_timings()
        assert call(n=0, d=padded.ptr, step=w + 5, win=0, nbytes=0) == 0
        assert ctx.timings() == {}
    finally:
        ctx.set_timing(0)
    padded.invalidate_host()
    assert not padded.host()[:, :w].any() and (padded.host()[:, w:] == 0xAB).all()
