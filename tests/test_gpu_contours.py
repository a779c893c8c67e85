"""Mask.to_disconnected_polygons on the GPU (csrc/contours.hip, vkx_mask_contours_dev): the batched call, the binding and the
element layer against the plain-Python restatement of cv.findContours(RETR_TREE) filtered to parent -1
(tests/contours_restate.py).  Every comparison is exact, the order of the contours included.

The labelling kernel works on tiles of 32 x 8 pixels (kTW x kTH of contours.hip) and the start compaction on chunks of 256 words
of 64 pixels; the shapes below are the smallest that cross those sizes."""
import logging
import os
import sys
from ctypes import c_void_p

import numpy as np
import pytest
from numpy.random import default_rng

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contours_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu

TILE_W, TILE_H = 32, 8
COMPACT_CHUNK = 256 * 64
METHODS = (R.CHAIN_APPROX_NONE, R.CHAIN_APPROX_SIMPLE)


def check(masks, methods=METHODS):
    """every mask of the list, in one batched call a method, against the restatement"""
    from vkit_amd import _native as N
    ctx = N.default_ctx()
    masks = [np.ascontiguousarray(m, dtype=np.uint8) for m in masks]
    planes = [ctx.to_device(m) for m in masks]
    for method in methods:
        got = N.mask_contours(planes, method)
        assert len(got) == len(masks)
        for mask, contours in zip(masks, got):
            R.same_contours(contours, R.contours(mask, method))
            assert all(c.dtype == np.int32 for c in contours)


def bands(h, w, dx, dy, period, width):
    y, x = np.mgrid[:h, :w]
    return ((dx * x + dy * y) % period < width).astype(np.uint8)


@pytest.mark.parametrize('shape', [(70, 150), (33, 257)])
def test_tile_seams(shape):
    """components (foreground and background) that cross every seam of the 32 x 8 labelling tiles: slanted bands both ways,
    their union (a lattice with holes), long rows and columns, and blobs"""
    h, w = shape
    assert h > 4 * TILE_H and w > 4 * TILE_W
    rng = default_rng(h)
    rows = np.zeros(shape, np.uint8)
    rows[TILE_H - 1::TILE_H] = 1                        # the last row of every tile: united with the next tile by NW / N / NE alone
    rows[:, ::5] |= np.uint8(rng.random((h, (w + 4) // 5)) < 0.5)
    columns = np.zeros(shape, np.uint8)
    columns[:, TILE_W - 1::TILE_W] = 1
    columns[1::3] |= np.uint8(rng.random((len(range(1, h, 3)), w)) < 0.3)
    masks = [bands(h, w, 1, 2, 9, 3), bands(h, w, 1, -3, 11, 2), bands(h, w, 1, 2, 9, 3) | bands(h, w, 1, -3, 11, 2), rows, columns,
             R.random_mask(default_rng(3), h, w, blobs=True), 1 - bands(h, w, 2, 1, 13, 1)]
    masks.append(np.uint8(rng.random(shape) < 0.5))
    check(masks)


def serpentine(n):
    """one component, 1 pixel wide with 1 pixel gaps, over the whole n x n plane"""
    mask = np.zeros((n, n), np.uint8)
    mask[::2] = 1
    for k, y in enumerate(range(1, n, 2)):
        mask[y, n - 1 if k % 2 == 0 else 0] = 1
    return mask


def test_long_merge_chains():
    """the serpentine needs the longest chain of merges across tiles; its inverse is the same for the background, whose walls
    make one hole-free foreground component each"""
    snake = serpentine(96)
    assert len(R.contours(snake)) == 1
    check([snake, 1 - snake, snake.T.copy(), (1 - snake).T.copy()])


def test_nesting():
    """three nested rings with an island in the innermost hole: only the outermost ring; a hole that touches the plane's edge by
    a corner only stays a hole (background is 4-connected)"""
    rings = np.zeros((41, 45), np.uint8)
    for k in (2, 7, 12):
        rings[k:41 - k, k:45 - k] = 1
        rings[k + 2:41 - k - 2, k + 2:45 - k - 2] = 0
    rings[20, 22] = 1
    assert len(R.contours(rings)) == 1
    corner = np.ones((12, 40), np.uint8)
    corner[0, 0] = 0                         # background on the edge
    corner[1, 1] = 0                         # touches it by a corner only: a hole
    corner[2:5, 2:5] = 0
    corner[3, 3] = 1                         # an island in that hole: not returned
    corner[11, 39] = 0
    corner[10, 38] = 0
    corner[6:9, 20:30] = 0
    corner[7, 22:28] = 1
    assert len(R.contours(corner)) == 1
    # an island in a hole that IS open to the edge through a 4-connected channel is returned
    channel = rings.copy()
    channel[20, :24] = 0
    channel[20, 22] = 1
    assert len(R.contours(channel)) > 1
    check([rings, corner, channel, np.pad(rings, 1), np.pad(corner, ((0, 3), (5, 0)))])


def test_diagonal_connectivity():
    board = np.uint8(np.indices((31, 31)).sum(axis=0) % 2 == 0)
    assert len(R.contours(board)) == 1
    check([board, 1 - board, np.pad(board, 2)])


def test_degenerate_planes():
    rng = default_rng(5)
    corners = np.zeros((9, 37), np.uint8)
    corners[0, 0] = corners[0, -1] = corners[-1, 0] = corners[-1, -1] = 1
    masks = [np.zeros((1, 1)), np.ones((1, 1)), np.zeros((1, 64)), np.ones((1, 64)), np.zeros((64, 1)), np.ones((64, 1)),
             rng.random((1, 64)) < 0.5, rng.random((64, 1)) < 0.5, np.zeros((20, 50)), np.ones((20, 50)), corners,
             np.full((3, 3), 255), np.ones((2, 2)), np.eye(2), np.eye(40)[:, ::-1]]
    check(masks)


def blobs_plane():
    """300 isolated 3 x 3 blobs on a plane of more pixels than one compaction chunk, then 20 single pixels and 20 pairs"""
    plane = np.zeros((136, 160), np.uint8)
    for k in range(300):
        y, x = 8 * (k // 20), 8 * (k % 20)
        plane[y + 1:y + 4, x + 2:x + 5] = 1
    for k in range(20):
        plane[122, 8 * k + 3] = 1
        plane[128, 8 * k + 1:8 * k + 3] = 1
    assert plane.size > COMPACT_CHUNK and plane[:88].size < COMPACT_CHUNK < plane[:120].size      # blobs on both sides of the chunk edge
    return plane


def test_many_starts():
    """starts compacted past one workgroup chunk, in raster order; contours of 1 and 2 points are in the raw call and dropped by
    the element layer"""
    from vkit_amd import _native as N
    from vkit_amd.element import Mask
    plane = blobs_plane()
    check([plane])
    ctx = N.default_ctx()
    dev = ctx.to_device(plane)
    raw = N.mask_contours_raw(N.contour_mask_records([dev]), R.CHAIN_APPROX_SIMPLE, ctx=ctx)
    assert raw.n_contours.tolist() == [340] and raw.status.tolist() == [0]
    lengths = raw.contour_len[:340].tolist()
    assert lengths == [4] * 300 + [1] * 20 + [2] * 20
    assert raw.totals.tolist() == [[340, 1260]]
    assert raw.contour_off[:340].tolist() == np.concatenate([[0], np.cumsum(lengths)[:-1]]).tolist()
    polygons = Mask(mat=dev).to_disconnected_polygons()
    assert len(polygons) == 300
    assert polygons[0].to_np_array().tolist() == [[2, 1], [2, 3], [4, 3], [4, 1]]


def page_and_windows(n, rng):
    """a page plane of set pixels with n windows of mixed shapes cut into it: a window's content is its own, what surrounds it
    is foreground that must not leak in"""
    page = np.ones((330, 331), np.uint8)
    windows, contents = [], []
    y = 1
    shapes = [(1, 1), (1, 40), (40, 1), (8, 32), (9, 33), (17, 65), (3, 100)] + [(int(rng.integers(2, 30)), int(rng.integers(2, 70)))
                                                                             for _ in range(n - 7)]
    x, row_h = 1, 0
    for h, w in shapes:
        if x + w + 1 > page.shape[1]:
            x, y, row_h = 1, y + row_h + 1, 0
        content = (rng.random((h, w)) < rng.uniform(0.2, 0.9)).astype(np.uint8)
        page[y:y + h, x:x + w] = content
        windows.append((y, x, h, w))
        contents.append(content)
        x, row_h = x + w + 1, max(row_h, h)
    assert y + row_h < page.shape[0]
    return page, windows, contents


def test_batch_of_windows_in_a_page():
    from vkit_amd import _native as N
    page, windows, contents = page_and_windows(70, default_rng(70))
    ctx = N.default_ctx()
    dev = ctx.to_device(page)
    for method in METHODS:
        got = N.mask_contours([(dev, up, left, h, w) for up, left, h, w in windows], method)
        assert len(got) == 70
        for content, contours in zip(contents, got):
            R.same_contours(contours, R.contours(content, method))


def test_more_masks_than_one_call():
    """a list of more than 4096 masks (the limit of one call) is split by the binding"""
    from vkit_amd import _native as N
    page = (default_rng(4).random((12, 90)) < 0.5).astype(np.uint8)
    n = N.CONTOURS_MAX_MASKS + 5
    windows = [(k % 9, k % 83, 3, 7) for k in range(n)]
    dev = N.default_ctx().to_device(page)
    got = N.mask_contours([(dev,) + window for window in windows])
    assert len(got) == n
    want = {}
    for (up, left, h, w), contours in zip(windows, got):
        if (up, left) not in want:
            want[up, left] = R.contours(page[up:up + h, left:left + w])
        R.same_contours(contours, want[up, left])


def test_capacity():
    """cap_points and cap_contours each one short: totals exact, status says so, nothing written; the binding's retry is whole"""
    from vkit_amd import _native as N
    rng = default_rng(9)
    masks = [R.random_mask(rng, 40, 60, blobs=k % 2 == 0) for k in range(6)] + [np.zeros((5, 5), np.uint8)]
    ctx = N.default_ctx()
    planes = [ctx.to_device(m) for m in masks]
    records = N.contour_mask_records(planes)
    for method in METHODS:
        want = [R.contours(m, method) for m in masks]
        totals = [[len(cs), sum(len(c) for c in cs)] for cs in want]
        need_contours, need_points = (sum(col) for col in zip(*totals))
        assert need_contours > 7 and need_points > need_contours
        exact = N.mask_contours_raw(records, method, need_contours, need_points, ctx)
        assert exact.totals.tolist() == totals and not exact.status.any()
        assert exact.n_contours.tolist() == [t[0] for t in totals]
        for caps in ((need_contours - 1, need_points), (need_contours, need_points - 1), (0, 0)):
            short = N.mask_contours_raw(records, method, *caps, ctx)
            assert short.totals.tolist() == totals
            assert short.status.tolist() == [N.CONTOURS_SHORT] * len(masks)
            assert not short.n_contours.any()
        for caps in ((need_contours - 1, None), (None, need_points - 1), (1, 1)):
            got = N.mask_contours(planes, method, cap_contours=caps[0], cap_points=caps[1])
            for contours, cs in zip(got, want):
                R.same_contours(contours, cs)


def _count(monkeypatch, ctx, call):
    from vkit_amd import _native as N
    syncs = []
    real = N.Context.sync
    ctx.sync()
    with monkeypatch.context() as m:
        m.setattr(N.Context, 'sync', lambda s: syncs.append(1) or real(s))
        ctx.set_timing(1)
        try:
            ctx.reset_timings()
            out = call()
            n_syncs = len(syncs)
            timings = ctx.timings()
        finally:
            ctx.set_timing(0)
    return out, {name: cnt for name, (_ms, cnt) in timings.items()}, n_syncs


KERNELS = ('k_contour_label_tiles', 'k_contour_merge', 'k_contour_flags', 'k_contour_compact', 'k_contour_mask_scan',
           'k_contour_trace_count', 'k_contour_offsets', 'k_contour_trace_write')


def test_launch_and_sync_budgets(monkeypatch):
    """device-resident batches of 1 and of 70 masks: the same eight launches, one synchronisation"""
    from vkit_amd import _native as N
    from vkit_amd.element import Mask
    from vkit_amd.element.mask import masks_to_disconnected_polygons
    ctx = N.default_ctx()
    rng = default_rng(1)
    seen = []
    for n in (1, 70):
        masks = [Mask(mat=ctx.to_device(R.random_mask(rng, 30, 50, blobs=True))) for _ in range(n)]
        masks_to_disconnected_polygons(masks)                  # warm the scratch slots
        _, launches, syncs = _count(monkeypatch, ctx, lambda: masks_to_disconnected_polygons(masks))
        seen.append([launches, syncs])
    assert seen[0] == seen[1] == [{name: 1 for name in KERNELS}, 1], seen


def test_abi_refusals():
    """every refusal of include/vkx.h: VKX_ERR_INVALID, nothing launched"""
    from vkit_amd import _native as N
    ctx, L = N.default_ctx(), N.lib()
    plane = ctx.to_device(np.ones((8, 9), np.uint8))
    out = ctx.dev_empty((4096,), np.uint8)
    names = ('n_contours', 'contour_len', 'contour_off', 'points', 'totals', 'status')
    base = dict(zip(names, (out.ptr, out.ptr + 256, out.ptr + 512, out.ptr + 1024, out.ptr + 2048, out.ptr + 3072)))

    def record(**over):
        rec = np.zeros(1, N.CONTOUR_MASK_DTYPE)
        rec['mask'], rec['step'], rec['h'], rec['w'] = plane.ptr, 9, 8, 9
        for key, value in over.items():
            rec[key] = value
        return rec

    def call(rec=None, n=1, method=2, cap_contours=16, cap_points=64, no_table=False, **over):
        rec = record() if rec is None else rec
        ptrs = dict(base, **over)
        return L.vkx_mask_contours_dev(ctx.handle, None if no_table else rec.ctypes.data, n, method, cap_contours, cap_points,
                                       *(c_void_p(ptrs[k]) if ptrs[k] else None for k in names))

    ctx.sync()
    ctx.set_timing(1)
    try:
        ctx.reset_timings()
        assert call(no_table=True) == -1
        for name in names:
            assert call(**{name: 0}) == -1, name
        assert call(record(mask=0)) == -1
        assert call(n=0) == -1 and call(n=-1) == -1 and call(n=4097) == -1
        assert call(record(h=0)) == -1 and call(record(w=0)) == -1 and call(record(h=32768)) == -1 and call(record(w=-3)) == -1
        assert call(record(step=8)) == -1 and call(record(step=-9)) == -1
        assert call(method=0) == -1 and call(method=3) == -1 and call(method=4) == -1
        assert call(cap_contours=-1) == -1 and call(cap_points=-1) == -1
        assert call(contour_off=base['contour_len'] + 4) == -1 and 'overlap' in N.last_error()
        assert call(points=base['totals'] - 8) == -1 and call(status=base['n_contours']) == -1
        assert call(record(mask=out.ptr + 1024 + 8)) == -1 and 'overlap' in N.last_error()        # a mask inside `points`
        assert call(totals=plane.ptr + 8) == -1
        assert ctx.timings() == {}
        assert call() == 0 and call(record(step=0, h=1)) == 0 and call(cap_contours=0, cap_points=0) == 0
        ctx.sync()
        assert {name: cnt for name, (_ms, cnt) in ctx.timings().items()} == {name: 3 for name in KERNELS}
    finally:
        ctx.set_timing(0)


# ---- the element layer ---------------------------------------------------------------------------------------------------------
def polygon_lists(polygons):
    return [[(int(x), int(y)) for x, y in polygon.to_np_array().tolist()] for polygon in polygons]


def shifted(contours, box):
    return [[(int(x) + box.left, int(y) + box.up) for x, y in c] for c in contours if len(c) >= 3]


def test_to_disconnected_polygons_on_a_boxed_resident_mask():
    from vkit_amd import _native as N
    from vkit_amd.element import Box, Mask
    ctx = N.default_ctx()
    mat = R.random_mask(default_rng(21), 50, 70, blobs=True)
    mat[:2, :5] = [[1, 0, 1, 1, 0], [0, 0, 0, 0, 0]]                           # contours of 1 and 2 points: dropped
    box = Box(up=13, down=13 + mat.shape[0] - 1, left=40, right=40 + mat.shape[1] - 1)
    for method in METHODS:
        want = shifted(R.contours(mat, method), box)
        assert len(want) < len(R.contours(mat, method))
        resident = Mask(mat=ctx.to_device(mat), box=box)
        assert polygon_lists(resident.to_disconnected_polygons(method)) == want
        assert resident.on_device
        assert polygon_lists(Mask(mat=mat, box=box).to_disconnected_polygons(cv_find_contours_method=method)) == want
    assert polygon_lists(Mask(mat=mat).to_disconnected_polygons()) == shifted(R.contours(mat), Box(up=0, down=0, left=0, right=0))


def test_to_external_polygon(caplog):
    from vkit_amd import _native as N
    from vkit_amd.element import Mask
    ctx = N.default_ctx()
    mat = np.zeros((30, 40), np.uint8)
    mat[2:6, 3:9] = 1
    mat[10:25, 12:35] = 1
    with caplog.at_level(logging.WARNING):
        polygon = Mask(mat=ctx.to_device(mat)).to_external_polygon()
    assert polygon.to_np_array().tolist() == [[12, 10], [12, 24], [34, 24], [34, 10]]
    assert 'More than one polygons is detected, keep the largest one as the external polygon.' in caplog.text
    single = np.zeros((30, 40), np.uint8)
    single[2:6, 3:9] = 1
    assert Mask(mat=single).to_external_polygon(R.CHAIN_APPROX_NONE).num_points == 16
    with pytest.raises(RuntimeError, match='Cannot find any contour.'):
        Mask(mat=ctx.to_device(np.zeros((30, 40), np.uint8))).to_external_polygon()


def test_to_disconnected_polygon_mask_pairs():
    from vkit_amd import _native as N
    from vkit_amd.element import Box, Mask
    import oracle as O
    ctx = N.default_ctx()
    mat = R.random_mask(default_rng(33), 40, 60, blobs=True)
    box = Box(up=5, down=5 + mat.shape[0] - 1, left=7, right=7 + mat.shape[1] - 1)
    want = shifted(R.contours(mat), box)
    pairs = Mask(mat=ctx.to_device(mat), box=box).to_disconnected_polygon_mask_pairs()
    assert polygon_lists([polygon for polygon, _ in pairs]) == want and len(want) >= 2
    for (polygon, mask), points in zip(pairs, want):
        xs, ys = [p[0] for p in points], [p[1] for p in points]
        assert (mask.box.up, mask.box.down, mask.box.left, mask.box.right) == (min(ys), max(ys), min(xs), max(xs))
        relative = np.array(points, np.int32) - np.array([min(xs), min(ys)], np.int32)
        raster = O.fill_poly(mask.shape, relative)
        assert (np.asarray(mask.mat) == (np.asarray(raster) > 0)).all()


def pair_masks(rng, resident):
    from vkit_amd import _native as N
    from vkit_amd.element import Box, Mask
    up, left = int(rng.integers(0, 50)), int(rng.integers(0, 50))
    a = R.random_mask(rng, 40, 90, blobs=True)
    a[a.shape[0] // 2, :] = 1
    h, w = a.shape
    a_box = Box(up=up, down=up + h - 1, left=left, right=left + w - 1)
    b_h, b_w = int(rng.integers(1, 40)), int(rng.integers(1, 90))
    b_up, b_left = up + int(rng.integers(-b_h + 1, h)), left + int(rng.integers(-b_w + 1, w))
    b_up, b_left = max(b_up, 0), max(b_left, 0)
    b = (rng.random((b_h, b_w)) < 0.8).astype(np.uint8)
    b_box = Box(up=b_up, down=b_up + b_h - 1, left=b_left, right=b_left + b_w - 1)
    if b_box.down < a_box.up or b_box.right < a_box.left:
        return pair_masks(rng, resident)
    hold = (lambda m: N.default_ctx().to_device(m)) if resident else (lambda m: m)
    box = Box(up=max(a_box.up, b_box.up), down=min(a_box.down, b_box.down), left=max(a_box.left, b_box.left),
              right=min(a_box.right, b_box.right))
    crop = lambda m, mb: m[box.up - mb.up:box.down - mb.up + 1, box.left - mb.left:box.right - mb.left + 1]  # noqa: E731
    want = shifted(R.contours(crop(a, a_box) & crop(b, b_box)), box)
    return Mask(mat=hold(a), box=a_box), Mask(mat=hold(b), box=b_box), want


@pytest.mark.parametrize('resident', [False, True])
def test_generate_precise_text_region_candidate_polygons(resident, monkeypatch):
    """singular and plural against numpy `&` plus the restatement; the plural form makes one contour call"""
    from vkit_amd import _native as N
    from vkit_amd.pipeline.text_detection import PageTextRegionStep
    rng = default_rng(44 + resident)
    cases = [pair_masks(rng, resident) for _ in range(12)]
    assert sum(bool(want) for _, _, want in cases) >= 6
    for precise, region, want in cases[:4]:
        assert polygon_lists(PageTextRegionStep.generate_precise_text_region_candidate_polygons(precise, region)) == want
    calls = []
    real = N.mask_contours_raw
    monkeypatch.setattr(N, 'mask_contours_raw', lambda *a, **k: calls.append(1) or real(*a, **k))
    got = PageTextRegionStep.generate_precise_text_region_candidate_polygons_of_pairs([(p, r) for p, r, _ in cases])
    assert calls == [1]
    assert [polygon_lists(polygons) for polygons in got] == [want for _, _, want in cases]


def test_random_sweep():
    """200 seeded masks up to 120 x 200, densities 0.05 .. 0.95, every fourth dilated into blobs, one batch a method"""
    rng = default_rng(2024)
    masks = [R.random_mask(rng, 120, 200, blobs=k % 4 == 3) for k in range(200)]
    assert max(m.shape[0] for m in masks) > 100 and max(m.shape[1] for m in masks) > 180
    check(masks)
