"""The bounding extended text-region masks on the GPU (TextRegionFlattener.get_bounding_extended_text_region_masks in
vkit_amd/pipeline/text_detection/page_text_region.py, csrc/region_masks.hip): the public classmethod against the reference's own
runs (tests/golden/text_region_masks.npz) on host and device-resident results, the classmethod and the raw entry point (with a
pitched text mask) against the numpy restatement (tests/text_region_masks_restate.py) on fresh seeds, the launch and
synchronisation budgets, the masks fed straight into build_flattened_text_regions, the ABI refusals.  Every comparison is exact."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_region_flatten_restate as F  # noqa: E402
import text_region_masks_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN_RUNS, _ = R.load_golden()


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
    assert got.tobytes() == want.tobytes()


def polygon_of(points):
    from vkit_amd.element import Polygon
    return Polygon.from_xy_pairs([(int(x), int(y)) for x, y in points])


def points_of(polygon):
    return np.array([(p.x, p.y) for p in polygon.points], np.int32)


def masks_equal(got, want, resident):
    """got: the Masks of the classmethod; want: [(mat, (up, down, left, right))]"""
    from vkit_amd import _native as N
    assert len(got) == len(want)
    for mask, (mat, box) in zip(got, want):
        assert isinstance(mask.arr, N.DevArray) == resident
        assert (mask.box.up, mask.box.down, mask.box.left, mask.box.right) == tuple(box)
        same(mask.mat, mat)


def fresh_case(shape, n, seed=0):
    """a fresh page (not a golden seed): the regions, their angles, every second region typical, and the restated masks with
    the rectangles patched by the host mirror (pinned against the reference in test_text_region_masks_golden.py)"""
    regions, angles = R.make_case(R.case_rng(shape, n, seed, base=5_000_000), shape, n)
    typical = list(range(0, n, 2))
    rectangles = [r if k in typical else points_of(polygon_of(d).to_bounding_rectangular_polygon(shape, angles[k]))
                  for k, (_, d, r) in enumerate(regions)]
    want = R.extended_masks(shape, [o for o, _, _ in regions], [d for _, d, _ in regions], rectangles)
    return regions, angles, typical, rectangles, want


def call_public(shape, regions, typical, angles):
    from vkit_amd.pipeline.text_detection import TextRegionFlattener
    return TextRegionFlattener.get_bounding_extended_text_region_masks(
        shape, [polygon_of(o) for o, _, _ in regions], [polygon_of(d) for _, d, _ in regions],
        [polygon_of(r) for _, _, r in regions], typical, angles)


@pytest.mark.parametrize('resident', [False, True])
@pytest.mark.parametrize('k', range(len(GOLDEN_RUNS)))
def test_classmethod_against_the_golden(k, resident):
    from vkit_amd import _native as N
    run = GOLDEN_RUNS[k]
    regions = [(g['original'], g['dilated'], g['rectangle']) for g in run['regions']]
    with N.resident(resident):
        got = call_public(tuple(run['shape']), regions, run['typical'], run['angles'])
        masks_equal(got, [(m['mat'], m['box']) for m in run['masks']], resident)


@pytest.mark.parametrize('resident', [False, True])
@pytest.mark.parametrize('shape', R.PAGES)
@pytest.mark.parametrize('n', R.COUNTS)
def test_classmethod_against_the_restatement(shape, n, resident):
    from vkit_amd import _native as N
    regions, angles, typical, _, want = fresh_case(shape, n)
    with N.resident(resident):
        masks_equal(call_public(shape, regions, typical, angles), want, resident)
        # no typical region at all: no rectangle is patched
        plain = R.extended_masks(shape, [o for o, _, _ in regions], [d for _, d, _ in regions], [r for _, _, r in regions])
        masks_equal(call_public(shape, regions, [], angles), plain, resident)


def test_classmethod_without_regions():
    from vkit_amd.pipeline.text_detection import TextRegionFlattener
    assert TextRegionFlattener.get_bounding_extended_text_region_masks((9, 9), [], [], [], [], []) == []


# ---- the raw entry point -----------------------------------------------------------------------------------------------
def raw_tables(originals, dilated, rectangles):
    """REGION_MASKS_REC_DTYPE records, the point table, the dense offsets and the size of the packed destination"""
    from vkit_amd import _native as N
    records = np.zeros(len(originals), N.REGION_MASKS_REC_DTYPE)
    tables, at, total = [], 0, 0
    for rec, o, d, r in zip(records, originals, dilated, rectangles):
        box = R.union_box(R.bounding_box(d), R.bounding_box(r))
        rec['up'], rec['down'], rec['left'], rec['right'] = box
        for name, points in (('o', o), ('d', d), ('r', r)):
            rec[name + '_off'], rec[name + '_cnt'] = at, len(points)
            tables.append(np.asarray(points, np.int32).reshape(-1, 2))
            at += len(points)
        rec['dst_off'] = total
        total += ((box[1] - box[0] + 1) * (box[3] - box[2] + 1) + 255) & ~255
    return records, np.ascontiguousarray(np.concatenate(tables, axis=0)), total


def unpack(host, records):
    out = []
    for rec in records:
        h, w = int(rec['down'] - rec['up'] + 1), int(rec['right'] - rec['left'] + 1)
        off = int(rec['dst_off'])
        out.append(host[off:off + h * w].reshape(h, w))
    return out


@pytest.mark.parametrize('shape', R.PAGES)
@pytest.mark.parametrize('n', R.COUNTS)
def test_entry_point_with_a_pitched_text_mask(shape, n):
    """the text mask as a rectangle of a wider plane, with values other than 1 where it is set; dst poisoned before the call:
    every byte of every output rectangle is written"""
    from vkit_amd import _native as N
    ctx = N.default_ctx()
    regions, _, _, rectangles, want = fresh_case(shape, n, seed=1)
    originals, dilated = [o for o, _, _ in regions], [d for _, d, _ in regions]
    T = R.text_mask(shape, originals)
    wide = np.full((shape[0], shape[1] + 13), 1, np.uint8)          # (set outside the page columns: must not be read as the page)
    wide[:, :shape[1]] = T * np.uint8(200)
    text = ctx.to_device(wide)
    records, points, total = raw_tables(originals, dilated, rectangles)
    dst = ctx.to_device(np.full(total, 0xA5, np.uint8))
    N.region_extend_masks(records, points, text, dst, text_mask_step=shape[1] + 13)
    for got, (mat, _) in zip(unpack(np.array(dst.host()), records), want):
        same(got, mat)


def test_entry_point_reports_more_than_64_crossings():
    """a comb of 136 vertices crosses a scanline 68 times: VKX_ERR_UNSUPPORTED as in vkx_paint_polys_dev (the call waits for
    the flag), and a comb of 68 vertices (34 crossings) next to it is served by the same path"""
    from vkit_amd import _native as N
    ctx = N.default_ctx()
    shape = (61, 203)
    text = N.dev_zeros(shape, np.uint8, ctx)
    for teeth, ok in ((17, True), (34, False)):
        polygon = R.comb(5, 3, 12, 16, teeth)
        records, points, total = raw_tables([polygon], [polygon], [polygon])
        dst = ctx.dev_empty((total,), np.uint8)
        if ok:
            N.region_extend_masks(records, points, text, dst)
            same(unpack(np.array(dst.host()), records)[0], R.extended_masks(shape, [polygon], [polygon], [polygon], T=np.zeros(shape, np.bool_))[0][0])
        else:
            with pytest.raises(N.VkxError, match='64 edge crossings'):
                N.region_extend_masks(records, points, text, dst)
    ctx.sync()


# ---- budgets -----------------------------------------------------------------------------------------------------------
def _count(monkeypatch, ctx, call):
    from vkit_amd import _native as N
    syncs, downloads = [], []
    real_sync, real_download = N.Context.sync, N.Context.download
    ctx.sync()
    with monkeypatch.context() as m:
        m.setattr(N.Context, 'sync', lambda s: syncs.append(1) or real_sync(s))
        m.setattr(N.Context, 'download', lambda s, dptr, array: downloads.append(1) or real_download(s, dptr, array))
        ctx.set_timing(1)
        try:
            ctx.reset_timings()
            out = call()
            if out and not isinstance(out[0].arr, N.DevArray):
                assert all(isinstance(mask.arr, np.ndarray) for mask in out)
            n_syncs, n_downloads = len(syncs), len(downloads)
            timings = ctx.timings()
        finally:
            ctx.set_timing(0)
    return {name: cnt for name, (_ms, cnt) in timings.items()}, n_syncs, n_downloads


def test_launch_and_sync_budgets(monkeypatch):
    """3 and 70 regions of at most 64 vertices a polygon: the same launches; resident: no synchronisation and no download;
    host results: one download"""
    from vkit_amd import _native as N
    ctx = N.default_ctx()
    shape = (96, 128)
    seen = []
    for n in (3, 70):
        regions, angles, typical, _, _ = fresh_case(shape, n, seed=2)
        regions = [g for g in regions if max(len(p) for p in g) <= 64]
        assert len(regions) >= n - 1
        row = []
        for resident in (True, False):
            with N.resident(resident):
                call = lambda: call_public(shape, regions, typical, angles)  # noqa: E731
                call()                                # warm the scratch slots
                row.append(_count(monkeypatch, ctx, call))
        seen.append(row)
    launches = {'k_paint_outline': 1, 'k_paint_spans': 1, 'k_paint_resolve': 1, 'k_region_mask_outline': 1, 'k_region_mask_spans': 1,
                'k_region_mask_resolve': 1}
    assert seen[0] == seen[1] == [(launches, 0, 0), (launches, 0, 1)], seen


# ---- the chain ---------------------------------------------------------------------------------------------------------
def test_masks_flow_into_the_flattening():
    """resident masks of the classmethod handed to build_flattened_text_regions as they are, against host masks of the
    restatement handed to the same function: the same flattened images, masks and boxes"""
    from vkit_amd import _native as N
    from vkit_amd.element import Box, Image, Mask
    from vkit_amd.pipeline.text_detection import TextRegionFlattener
    shape, n = (96, 128), 70
    regions, angles, typical, _, want = fresh_case(shape, n, seed=3)
    page = np.random.default_rng(9).integers(0, 256, shape + (3,), dtype=np.uint8)
    # flattening angles under which no rotated mask comes out empty (the reference raises for those); empty masks are left out
    keep, flatten_angles = [], []
    for k, (mat, box) in enumerate(want):
        for angle in ((45, 90, 0)[k % 3], 90, 0):
            try:
                F.flatten(page, mat, box, angle)
            except RuntimeError:
                continue
            keep.append(k)
            flatten_angles.append(angle)
            break
    assert len(keep) > 50
    with N.resident(True):
        masks = call_public(shape, regions, typical, angles)
        assert all(isinstance(m.arr, N.DevArray) for m in masks)
        got = TextRegionFlattener.build_flattened_text_regions(Image(mat=page), [None] * len(keep), [masks[k] for k in keep], typical,
                                                               flatten_angles, None)
    host_masks = [Mask(mat=want[k][0], box=Box(up=want[k][1][0], down=want[k][1][1], left=want[k][1][2], right=want[k][1][3]))
                  for k in keep]
    ref = TextRegionFlattener.build_flattened_text_regions(Image(mat=page), [None] * len(keep), host_masks, typical, flatten_angles, None)
    assert len(got) == len(ref) == len(keep)
    for a, b in zip(got, ref):
        assert isinstance(a.flattened_image.arr, N.DevArray) and isinstance(b.flattened_image.arr, np.ndarray)
        same(a.flattened_image.mat, b.flattened_image.mat)
        same(a.flattened_mask.mat, b.flattened_mask.mat)
        assert a.rotated_trimmed_box == b.rotated_trimmed_box and a.shape_before_trim == b.shape_before_trim
        assert a.bounding_extended_text_region_mask.box == b.bounding_extended_text_region_mask.box


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_abi_refusals():
    """every refusal of include/vkx.h is VKX_ERR_INVALID with nothing launched, and a clean call on the same context afterwards
    still matches"""
    from ctypes import c_void_p
    from vkit_amd import _native as N
    ctx, L = N.default_ctx(), N.lib()
    shape = (96, 128)
    regions, _, _, rectangles, want = fresh_case(shape, 3, seed=4)
    originals, dilated = [o for o, _, _ in regions], [d for _, d, _ in regions]
    text = ctx.to_device(R.text_mask(shape, originals).astype(np.uint8))
    records, points, total = raw_tables(originals, dilated, rectangles)
    dst = ctx.dev_empty((total,), np.uint8)
    INVALID = -1                                       # VKX_ERR_INVALID

    def call(recs=records, n=None, pts=points, t=text.ptr, step=shape[1], h=shape[0], w=shape[1], d=dst.ptr, nbytes=total):
        return L.vkx_region_extend_masks_dev(ctx.handle, recs.ctypes.data if recs is not None else None, len(records) if n is None else n,
                                             pts.ctypes.data if pts is not None else None, c_void_p(t) if t else None, step, h, w,
                                             c_void_p(d) if d else None, nbytes)

    def edited(k=0, **over):
        recs = records.copy()
        for key, value in over.items():
            recs[k][key] = value
        return recs

    def moved(index, xy):
        pts = points.copy()
        pts[index] = xy
        return pts

    ctx.set_timing(1)
    try:
        ctx.reset_timings()
        refused = [
            call(recs=None), call(pts=None), call(t=0), call(d=0),                                      # NULL pointers
            call(n=0), call(n=-1), call(n=4097),                                                        # the count
            call(recs=edited(down=shape[0])), call(recs=edited(right=shape[1])), call(recs=edited(up=-1)),   # BB outside the page
            call(recs=edited(left=int(records[0]['right']) + 1)),                                       # a side of 0
            call(recs=edited(up=0, down=32767), h=40000),                                               # a side of 32768
            call(recs=edited(o_cnt=0)), call(recs=edited(d_cnt=0)), call(recs=edited(r_cnt=-3)), call(recs=edited(r_off=-1)),
            call(pts=moved(int(records[0]['o_off']), (int(records[0]['right']) + 1, int(records[0]['up'])))),   # O leaves BB
            call(pts=moved(int(records[1]['r_off']), (int(records[1]['left']), int(records[1]['up']) - 1))),
            call(nbytes=total - 256), call(recs=edited(k=2, dst_off=-1)),                               # a destination outside dst
            call(recs=edited(k=1, dst_off=int(records[0]['dst_off']))),                                  # overlapping destinations
            call(t=dst.ptr), call(d=text.ptr + 64, nbytes=64),                                          # the text mask over dst
            call(step=shape[1] - 1), call(step=-shape[1]),                                              # the row step
        ]
        assert refused == [INVALID] * len(refused), refused
        assert ctx.timings() == {}                     # nothing was launched
    finally:
        ctx.set_timing(0)
    assert call() == 0
    for got, (mat, _) in zip(unpack(np.array(dst.host()), records), want):
        same(got, mat)
