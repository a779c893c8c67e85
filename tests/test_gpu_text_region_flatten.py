"""The pixel half of PageTextRegionStep on the GPU (vkit_amd/pipeline/text_detection/page_text_region.py,
csrc/region_flatten.hip): the public functions against the reference's own runs (tests/golden/text_region_flatten.npz) on host and
device-resident pages, the public functions and the four kernels against the numpy restatement
(tests/text_region_flatten_restate.py) on fixed seeds, the batched entry points against N calls of the single-pair entry points,
Mask.to_external_box on the device, the launch and synchronisation budgets, the ABI refusals.  Every comparison is exact."""
import os
import sys

import numpy as np
import pytest
from numpy.random import default_rng

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_region_flatten_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu

LUT_X255 = ((np.arange(256) > 0).astype(np.uint8) * 255).reshape(1, 256)
FLATTEN_ANGLES = (1, 45, 89, 90, 91, 135, 180, 269, 270, 359)
PAGES = ((96, 128), (61, 203))


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
    assert got.tobytes() == want.tobytes()


def make_page(rng, shape, n):
    """a page and n box-attached region masks: 1 x N, N x 1 and 5 .. 40 px boxes, one touching each page border, one mask of a
    single pixel, one full mask"""
    from vkit_amd.element import Box, Mask
    h, w = shape
    page = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    special = [(0, 0, 9, 17, 'rand'), (h - 7, 3, 7, 11, 'rand'), (5, 0, 12, 6, 'rand'), (2, w - 9, 8, 9, 'rand'),
               (10, 20, 9, 13, 'pixel'), (20, 30, 6, 21, 'full'), (30, 5, 1, 23, 'full'), (3, 40, 19, 1, 'full')]
    masks, angles = [], []
    for k in range(n):
        if n > 3 and k < len(special):
            up, left, bh, bw, kind = special[k]
        else:
            bh, bw = int(rng.integers(5, 41)), int(rng.integers(5, 41))
            up, left, kind = int(rng.integers(0, h - bh + 1)), int(rng.integers(0, w - bw + 1)), 'rand'
        if kind == 'full':
            mat = np.ones((bh, bw), np.uint8)
        elif kind == 'pixel':
            mat = np.zeros((bh, bw), np.uint8)
            mat[bh // 2, bw // 2] = 1
        else:
            mat = (rng.random((bh, bw)) < 0.8).astype(np.uint8)
            mat[bh // 2, bw // 2] = 1
        masks.append(Mask(mat=mat).to_box_attached(Box(up=up, down=up + bh - 1, left=left, right=left + bw - 1)))
        angles.append(FLATTEN_ANGLES[k % len(FLATTEN_ANGLES)])
    return page, masks, angles


def try_flatten(page, mask, angle):
    b = mask.box
    try:
        return R.flatten(page, mask.mat, (b.up, b.down, b.left, b.right), angle)
    except RuntimeError:
        return None


def usable(rng, shape, n):
    """make_page with the regions whose rotated mask comes out empty (a single pixel spread thin) turned by 90 degrees"""
    page, masks, angles = make_page(rng, shape, n)
    for k in range(n):
        if try_flatten(page, masks[k], angles[k]) is None:
            angles[k] = 90
    return page, masks, angles


@pytest.mark.parametrize('resident', [False, True])
@pytest.mark.parametrize('shape', PAGES)
@pytest.mark.parametrize('n', [1, 3, 70])
def test_public_functions_against_the_restatement(shape, n, resident):
    """build, resize (up, down, to a height of 1), post-rotate (0, 90, 180, 270) and stack on host and resident pages"""
    from vkit_amd import _native as N
    from vkit_amd.element import Image, Mask
    from vkit_amd.pipeline.text_detection import (ColumnPacker, TextRegionFlattener, post_rotate_flattened_text_regions,
                                                  resize_flattened_text_regions, stack_flattened_text_regions)
    rng = default_rng(1000 * n + shape[0])
    page, masks, angles = usable(rng, shape, n)
    ctx = N.default_ctx()
    image = Image(mat=ctx.to_device(page) if resident else page)
    if resident:
        masks = [Mask(mat=ctx.to_device(m.mat), box=m.box) for m in masks]
    with N.resident(resident):
        regions = TextRegionFlattener.build_flattened_text_regions(image, [None] * n, masks, range(0, n, 2), angles, None)
        want = [R.flatten(page, m.mat, (m.box.up, m.box.down, m.box.left, m.box.right), a) for m, a in zip(masks, angles)]
        assert len(regions) == n
        for k, (got, ref) in enumerate(zip(regions, want)):
            assert isinstance(got.flattened_image.arr, N.DevArray) == resident
            same(got.flattened_image.mat, ref['image'])
            same(got.flattened_mask.mat, ref['mask'])
            b = got.rotated_trimmed_box
            assert (b.up, b.down, b.left, b.right) == ref['rotated_trimmed_box']
            assert tuple(got.shape_before_trim) == ref['shape_before_trim'] and got.shape_before_resize == ref['image'].shape[:2]
            assert got.is_typical == (k % 2 == 0) and got.post_rotate_angle == 0 and got.flattening_rotate_angle == angles[k]
        same(regions[0].text_region_image.mat, page[masks[0].box.up:masks[0].box.down + 1, masks[0].box.left:masks[0].box.right + 1]
             * (masks[0].mat > 0)[:, :, None])
        # the stackable regions: image and mask of one shape (the reference's crop quirk can make them differ)
        keep = [k for k, r in enumerate(want) if r['image'].shape[:2] == r['mask'].shape]
        targets = []
        for k, r in enumerate(want):
            h, w = r['image'].shape[:2]       # (an aspect that would round the free side to 0 gets both sides)
            targets.append([(1, None if round(w / h) else 1), (None if round(7 * h / w) else 1, 7), (h + 3, w + 2),
                            (max(h // 2, 1), max(w // 3, 1))][k % 4])
        resized = resize_flattened_text_regions(regions, targets)
        want_resized = [R.resize_pair(r['image'], r['mask'], *t) for r, t in zip(want, targets)]
        for got, (ref_image, ref_mask) in zip(resized, want_resized):
            same(got.flattened_image.mat, ref_image)
            same(got.flattened_mask.mat, ref_mask)
        single = regions[0].to_resized_flattened_text_region(*targets[0])
        same(single.flattened_image.mat, want_resized[0][0])
        post = [(0, 90, 180, 270)[k % 4] for k in range(len(keep))]
        rotated = post_rotate_flattened_text_regions([resized[k] for k in keep], post)
        want_rotated = []
        for k, angle, got in zip(keep, post, rotated):
            ref = want_resized[k] if angle == 0 else R.post_rotate_pair(*want_resized[k], angle)
            want_rotated.append(ref)
            same(got.flattened_image.mat, ref[0])
            same(got.flattened_mask.mat, ref[1])
            assert got.post_rotate_angle == angle
            if angle == 0:
                assert got is resized[k]
        if not rotated:
            return
        stacked = stack_flattened_text_regions(1, 2, rotated, ColumnPacker)
        origins = [(b.up, b.left) for b in stacked[2]]
        assert origins[0] == (3, 3) and all(b.shape == r.shape for b, r in zip(stacked[2], rotated))
        page_shape = (max(b.down for b in stacked[2]) + 1 + 2 + 1, max(b.right for b in stacked[2]) + 1 + 2 + 1)
        want_image, want_active = R.stack(page_shape, want_rotated, origins)
        assert isinstance(stacked[0].arr, N.DevArray) == resident
        same(stacked[0].mat, want_image)
        same(stacked[1].mat, want_active)


def test_background_matches_the_reference_rows():
    from vkit_amd import _native as N
    from vkit_amd.pipeline.text_detection import build_background_image_for_stacking
    same(build_background_image_for_stacking(7, 11).mat, R.background(7, 11))
    with N.resident(True):
        same(build_background_image_for_stacking(7, 11).mat, R.background(7, 11))


def _random_pairs(rng, n):
    images, masks = [], []
    for _ in range(n):
        h, w = (int(v) for v in rng.integers(1, 41, 2))
        images.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        masks.append((rng.random((h, w)) < 0.7).astype(np.uint8))
    return images, masks


def _upload(ctx, arrays):
    return [ctx.to_device(a) for a in arrays]


def _layout(sizes):
    offsets, total = [], 0
    for s in sizes:
        offsets.append(total)
        total += (s + 255) & ~255
    return offsets, total


@pytest.mark.parametrize('n', [1, 257])
def test_warp_kernel_against_the_restatement_and_the_single_entry(n):
    """vkx_region_warp_dev on random tables: the restatement, and N calls of vkx_warp_affine_u8_dev (every pair)"""
    from vkit_amd import _native as N
    ctx = N.default_ctx()
    rng = default_rng(31 + n)
    images, masks = _random_pairs(rng, n)
    dimg, dmsk = _upload(ctx, images), _upload(ctx, masks)
    pairs = np.zeros(n, N.REGION_WARP_PAIR_DTYPE)
    mats, sizes = [], []
    for k in range(n):
        mat, dsize = R.rotate_matrix(int(rng.integers(0, 360)), masks[k].shape)
        mats.append((mat, dsize))
        sizes += [dsize[0] * dsize[1] * 3, dsize[0] * dsize[1]]
    offsets, total = _layout(sizes)
    dst = ctx.dev_empty((total,), np.uint8)
    for k, p in enumerate(pairs):
        h, w = masks[k].shape
        p['src_image'], p['src_mask'], p['src_image_step'], p['src_mask_step'] = dimg[k].ptr, dmsk[k].ptr, w * 3, w
        p['src_h'], p['src_w'], p['m'] = h, w, mats[k][0].reshape(6)
        p['dst_h'], p['dst_w'] = mats[k][1][1], mats[k][1][0]
        p['dst_image_off'], p['dst_mask_off'] = offsets[2 * k], offsets[2 * k + 1]
    for extract in (False, True):
        N.region_warp(pairs, extract, dst)
        host = np.array(dst.host())
        for k in range(n):
            dw, dh = mats[k][1]
            want_image, want_mask = R.warp_pair(images[k], masks[k], *mats[k], extract=extract)
            same(host[offsets[2 * k]:offsets[2 * k] + dh * dw * 3].reshape(dh, dw, 3), want_image)
            same(host[offsets[2 * k + 1]:offsets[2 * k + 1] + dh * dw].reshape(dh, dw), want_mask)
            if not extract:
                same(N.warp_affine(dimg[k], mats[k][0], mats[k][1]).host(), want_image)
                same(N.warp_affine(dmsk[k], mats[k][0], mats[k][1]).host(), want_mask)


@pytest.mark.parametrize('n', [1, 257])
def test_resize_and_extent_kernels_against_the_restatement_and_the_single_entry(n):
    from vkit_amd import _native as N
    ctx = N.default_ctx()
    rng = default_rng(57 + n)
    images, masks = _random_pairs(rng, n)
    for k in range(0, n, 5):
        masks[k][:] = 0                       # empty masks for the extent kernel
    dimg, dmsk = _upload(ctx, images), _upload(ctx, masks)
    targets = [tuple(int(v) for v in rng.integers(1, 61, 2)) for _ in range(n)]
    sizes = []
    for dh, dw in targets:
        sizes += [dh * dw * 3, dh * dw]
    offsets, total = _layout(sizes)
    dst = ctx.dev_empty((total,), np.uint8)
    pairs = np.zeros(n, N.REGION_RESIZE_PAIR_DTYPE)
    for k, p in enumerate(pairs):
        h, w = masks[k].shape
        p['src_image'], p['src_mask'], p['src_image_step'], p['src_mask_step'] = dimg[k].ptr, dmsk[k].ptr, w * 3, w
        p['src_h'], p['src_w'], p['dst_h'], p['dst_w'] = h, w, targets[k][0], targets[k][1]
        p['dst_image_off'], p['dst_mask_off'] = offsets[2 * k], offsets[2 * k + 1]
    N.region_resize(pairs, dst)
    host = np.array(dst.host())
    for k in range(n):
        dh, dw = targets[k]
        want_image, want_mask = R.resize_pair(images[k], masks[k], dh, dw)
        same(host[offsets[2 * k]:offsets[2 * k] + dh * dw * 3].reshape(dh, dw, 3), want_image)
        same(host[offsets[2 * k + 1]:offsets[2 * k + 1] + dh * dw].reshape(dh, dw), want_mask)
        # N calls of vkx_resize_cubic_u8_dev: the image as it is, the mask as (> 0) * 255, resized, > 0
        same(N.resize_cubic(dimg[k], (dh, dw)).host(), want_image)
        plane = N.resize_cubic(N.apply_lut(dmsk[k], LUT_X255), (dh, dw)).host()
        same((plane > 0).astype(np.uint8), want_mask)
    # the extents of the resized masks, packed as they are
    extents = np.array(N.region_extent(dst, offsets[1::2], targets).host())
    for k in range(n):
        _, want_mask = R.resize_pair(images[k], masks[k], *targets[k])
        want = R.external_box(want_mask) if want_mask.any() else (-1, -1, -1, -1)
        assert tuple(int(v) for v in extents[k]) == want, k


@pytest.mark.parametrize('shape', [(16, 64), (37, 150)])
@pytest.mark.parametrize('n', [1, 257])
def test_stack_kernel_against_the_restatement(n, shape):
    """vkx_region_stack_dev on random, overlapping boxes: where regions overlap the last in the caller's order wins.  A page of
    16 x 64 is ONE tile of the kernel, so at 257 regions more than its list of 256 meet it and every record is scanned; on
    37 x 150 the tiles list the regions that meet them."""
    from vkit_amd import _native as N
    ctx = N.default_ctx()
    rng = default_rng(91 + n + shape[0])
    h, w = shape
    regions, origins = [], []
    for _ in range(n):
        rh, rw = int(rng.integers(1, h + 1)), int(rng.integers(1, min(w, 40) + 1))
        regions.append((rng.integers(0, 256, (rh, rw, 3), dtype=np.uint8), (rng.random((rh, rw)) < 0.6).astype(np.uint8) * rng.integers(1, 256, dtype=np.uint8)))
        origins.append((int(rng.integers(0, h - rh + 1)), int(rng.integers(0, w - rw + 1))))
    dimg, dmsk = _upload(ctx, [r[0] for r in regions]), _upload(ctx, [r[1] for r in regions])
    items = np.zeros(n, N.REGION_STACK_ITEM_DTYPE)
    for k, item in enumerate(items):
        item['image'], item['mask'] = dimg[k].ptr, dmsk[k].ptr
        item['h'], item['w'] = regions[k][1].shape
        item['up'], item['left'] = origins[k]
    image, active = N.region_stack(items, shape, ctx=ctx)
    want_image, want_active = R.stack(shape, regions, origins)
    if n == 257:
        covered = np.zeros(shape, np.int32)
        for (_, mask), (up, left) in zip(regions, origins):
            covered[up:up + mask.shape[0], left:left + mask.shape[1]] += mask > 0
        assert covered.max() > 1                       # the boxes do overlap under set masks
    same(image.host(), want_image)
    same(active.host(), want_active)


@pytest.mark.parametrize('resident', [False, True])
def test_region_whose_image_and_mask_shapes_differ(resident):
    """Image.to_cropped_image takes `down or height - 1`: a rotated mask that occupies row 0 alone of a taller warped plane
    leaves the image untrimmed on that axis.  Such a region takes two records in the flattening and in the resize."""
    from vkit_amd import _native as N
    from vkit_amd.element import Box, Image, Mask
    from vkit_amd.pipeline.text_detection import TextRegionFlattener, resize_flattened_text_regions
    ctx = N.default_ctx()
    rng = default_rng(3)
    page = rng.integers(0, 256, (40, 50, 3), dtype=np.uint8)
    mats = [np.zeros((6, 9), np.uint8), np.ones((7, 5), np.uint8)]
    mats[0][:, 0] = 1                                  # its first column becomes row 0 of the plane turned by 90 degrees
    boxes = [(3, 8, 4, 12), (20, 26, 30, 34)]
    put = (lambda a: ctx.to_device(a)) if resident else (lambda a: a)
    masks = [Mask(mat=put(m), box=Box(up=b[0], down=b[1], left=b[2], right=b[3])) for m, b in zip(mats, boxes)]
    want = [R.flatten(page, m, b, 90) for m, b in zip(mats, boxes)]
    assert want[0]['image'].shape == (9, 6, 3) and want[0]['mask'].shape == (1, 6)          # the shapes really differ
    assert want[1]['image'].shape[:2] == want[1]['mask'].shape
    with N.resident(resident):
        built = TextRegionFlattener.build_flattened_text_regions(Image(mat=put(page)), [None, None], masks, (), [90, 90], None)
        for got, ref in zip(built, want):
            assert isinstance(got.flattened_image.arr, N.DevArray) == resident
            same(got.flattened_image.mat, ref['image'])
            same(got.flattened_mask.mat, ref['mask'])
        assert built[0].shape == (9, 6) and built[0].flattened_mask.shape == (1, 6) and built[0].shape_before_resize == (9, 6)
        for target in ((5, 11), (3, None)):
            resized = resize_flattened_text_regions(built, [target, target])
            for got, ref in zip(resized, want):
                ref_image, ref_mask = R.resize_pair(ref['image'], ref['mask'], *target)
                same(got.flattened_image.mat, ref_image)
                same(got.flattened_mask.mat, ref_mask)
        assert resized[0].flattened_image.shape != resized[0].flattened_mask.shape          # (3, None): each from its own aspect


def test_mask_to_external_box_on_the_device():
    from vkit_amd import _native as N
    from vkit_amd.element import Mask
    ctx = N.default_ctx()
    rng = default_rng(5)
    for shape in ((1, 1), (37, 203), (300, 5)):
        mat = (rng.random(shape) < 0.02).astype(np.uint8)
        mat[shape[0] // 2, shape[1] // 3] = 7
        host, dev = Mask(mat=mat).to_external_box(), Mask(mat=ctx.to_device(mat)).to_external_box()
        assert (dev.up, dev.down, dev.left, dev.right) == (host.up, host.down, host.left, host.right) == R.external_box(mat)
    for mask in (Mask(mat=np.zeros((9, 70), np.uint8)), Mask(mat=ctx.to_device(np.zeros((9, 70), np.uint8)))):
        with pytest.raises(RuntimeError, match='to_external_box: empty np_mask.'):
            mask.to_external_box()


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


def test_launch_and_sync_budgets(monkeypatch):
    """device-resident pages of 3 and of 70 regions: the same launches and synchronisations"""
    from vkit_amd import _native as N
    from vkit_amd.element import Image, Mask
    from vkit_amd.pipeline.text_detection import (ColumnPacker, TextRegionFlattener, post_rotate_flattened_text_regions,
                                                  resize_flattened_text_regions, stack_flattened_text_regions)
    ctx = N.default_ctx()
    seen = []
    for n in (3, 70):
        page, masks, angles = usable(default_rng(n), (96, 128), n)
        for k in range(n):
            angles[k] = (45, 90, 180)[k % 3] if angles[k] != 90 else 90
        page, masks, angles = page, masks, [a if try_flatten(page, m, a) else 90 for m, a in zip(masks, angles)]
        image = Image(mat=ctx.to_device(page))
        masks = [Mask(mat=ctx.to_device(m.mat), box=m.box) for m in masks]
        build = lambda: TextRegionFlattener.build_flattened_text_regions(image, [None] * n, masks, (), angles, None)  # noqa: E731
        build()                                   # warm the scratch slots
        regions, launches, syncs = _count(monkeypatch, ctx, build)
        row = [launches, syncs]
        regions = [r for r in regions if r.flattened_image.shape == r.flattened_mask.shape]
        resized, launches, syncs = _count(monkeypatch, ctx, lambda: resize_flattened_text_regions(regions, [(9, 14)] * len(regions)))
        row += [launches, syncs]
        rotated, launches, syncs = _count(monkeypatch, ctx, lambda: post_rotate_flattened_text_regions(
            resized, [(90, 0, 270)[k % 3] for k in range(len(resized))]))
        row += [launches, syncs]
        _, launches, syncs = _count(monkeypatch, ctx, lambda: stack_flattened_text_regions(0, 2, rotated, ColumnPacker))
        row += [launches, syncs]
        seen.append(row)
    assert seen[0] == seen[1] == [{'k_region_warp': 2, 'k_region_extent': 1}, 1, {'k_region_resize': 1}, 0, {'k_region_warp': 1}, 0,
                                  {'k_region_stack': 1}, 0], seen


def test_abi_refusals():
    """NULL tables, counts below range, a destination over its source, row steps shorter than a row: VKX_ERR_INVALID, nothing
    launched (include/vkx.h)"""
    from ctypes import c_void_p
    from vkit_amd import _native as N
    ctx, L = N.default_ctx(), N.lib()
    h = ctx.handle
    src_image, src_mask = ctx.to_device(np.zeros((8, 9, 3), np.uint8)), ctx.to_device(np.ones((8, 9), np.uint8))
    dst = ctx.dev_empty((4096,), np.uint8)

    def warp_pair(**over):
        p = np.zeros(1, N.REGION_WARP_PAIR_DTYPE)
        p['src_image'], p['src_mask'], p['src_image_step'], p['src_mask_step'] = src_image.ptr, src_mask.ptr, 27, 9
        p['src_h'], p['src_w'], p['m'], p['dst_h'], p['dst_w'] = 8, 9, (1, 0, 0, 0, 1, 0), 8, 9
        p['dst_image_off'], p['dst_mask_off'] = 0, 256
        for key, value in over.items():
            p[key] = value
        return p

    def resize_pair(**over):
        p = np.zeros(1, N.REGION_RESIZE_PAIR_DTYPE)
        for key in ('src_image', 'src_mask', 'src_image_step', 'src_mask_step', 'src_h', 'src_w', 'dst_h', 'dst_w', 'dst_image_off',
                    'dst_mask_off'):
            p[key] = warp_pair()[key]
        for key, value in over.items():
            p[key] = value
        return p

    def warp(p, n=1, d=dst, nbytes=4096):
        return L.vkx_region_warp_dev(h, p.ctypes.data if p is not None else None, n, 0, c_void_p(d.ptr) if d is not None else None, nbytes)

    def resize(p, n=1, d=dst, nbytes=4096):
        return L.vkx_region_resize_dev(h, p.ctypes.data if p is not None else None, n, c_void_p(d.ptr) if d is not None else None, nbytes)

    for call, pair in ((warp, warp_pair), (resize, resize_pair)):
        assert call(pair()) == 0
        assert call(None) != 0 and call(pair(), d=None) != 0
        assert call(pair(), n=-1) != 0 and call(pair(), n=0) != 0
        assert call(pair(src_image_step=26)) != 0 and call(pair(src_mask_step=8)) != 0 and call(pair(src_mask_step=-9)) != 0
        assert call(pair(src_mask=0)) != 0 and call(pair(src_image=0)) != 0
        assert call(pair(dst_image_off=4096 - 8)) != 0 and call(pair(dst_mask_off=100)) != 0      # outside dst; overlapping
        assert call(pair(dst_image_off=-1, dst_mask_off=-1)) != 0
        assert call(pair(dst_h=0)) != 0 and call(pair(src_w=40000)) != 0
        assert call(pair(src_image=dst.ptr + 1024)) != 0                                          # a source inside dst
        assert 'overlap' in N.last_error()
    offsets, shapes, out = np.zeros(1, np.int64), np.array([[8, 9]], np.int32), ctx.dev_empty((1, 4), np.int32)

    def extent(m=src_mask, nbytes=72, o=offsets, s=shapes, n=1, e=out):
        return L.vkx_region_extent_dev(h, c_void_p(m.ptr) if m is not None else None, nbytes, o.ctypes.data if o is not None else None,
                                       s.ctypes.data if s is not None else None, n, c_void_p(e.ptr) if e is not None else None)

    assert extent() == 0
    assert extent(m=None) != 0 and extent(o=None) != 0 and extent(s=None) != 0 and extent(e=None) != 0
    assert extent(n=-1) != 0 and extent(n=0) != 0 and extent(nbytes=71) != 0 and extent(o=np.array([-1], np.int64)) != 0
    assert extent(e=src_mask) != 0
    item = np.zeros(1, N.REGION_STACK_ITEM_DTYPE)
    item['image'], item['mask'], item['h'], item['w'], item['up'], item['left'] = src_image.ptr, src_mask.ptr, 8, 9, 2, 3
    page_image, page_mask = ctx.dev_empty((12, 12, 3), np.uint8), ctx.dev_empty((12, 12), np.uint8)

    def stack(it=item, n=1, pi=page_image, pm=page_mask, hh=12, ww=12):
        return L.vkx_region_stack_dev(h, it.ctypes.data if it is not None else None, n, c_void_p(pi.ptr) if pi is not None else None,
                                      c_void_p(pm.ptr) if pm is not None else None, hh, ww)

    assert stack() == 0 and stack(it=None, n=0) == 0
    assert stack(it=None) != 0 and stack(pi=None) != 0 and stack(pm=None) != 0 and stack(n=-1) != 0
    assert stack(ww=11) != 0 and stack(hh=9) != 0 and stack(hh=0) != 0                             # the box leaves the page
    assert stack(pm=page_image) != 0 and stack(pi=src_image, hh=2, ww=2, it=None, n=0) == 0
    bad = item.copy()
    bad['image'] = page_image.ptr
    assert stack(it=bad) != 0
    ctx.sync()


# ---- against the reference's own runs (tests/golden/text_region_flatten.npz) ------------------------------------------------
GOLDEN_RUNS, GOLDEN_BACKGROUND = R.load_golden()


def _chars_equal(polygons, want):
    if want is None:
        assert polygons is None
        return
    assert len(polygons) == len(want)
    for polygon, xy in zip(polygons, want):
        got = np.array([(p.smooth_x, p.smooth_y) for p in polygon.points], np.float64)
        same(got, xy)


def _region_equal(got, want, resident):
    from vkit_amd import _native as N
    assert isinstance(got.flattened_image.arr, N.DevArray) == resident
    same(got.flattened_image.mat, want['image'])
    same(got.flattened_mask.mat, want['mask'])
    b = got.rotated_trimmed_box
    assert [b.up, b.down, b.left, b.right] == want['rotated_trimmed_box']
    assert list(got.shape_before_trim) == want['shape_before_trim'] and list(got.shape_before_resize) == want['shape_before_resize']
    assert got.post_rotate_angle == want['post_rotate_angle'] and got.is_typical == want['is_typical']
    _chars_equal(got.flattened_char_polygons, want['chars'])


@pytest.mark.parametrize('resident', [False, True])
@pytest.mark.parametrize('k', range(len(GOLDEN_RUNS)))
def test_public_functions_against_the_golden(k, resident):
    from vkit_amd import _native as N
    from vkit_amd.element import Box, Image, Mask, Polygon
    from vkit_amd.pipeline.text_detection import (TextRegionFlattener, post_rotate_flattened_text_regions,
                                                  resize_flattened_text_regions, stack_flattened_text_regions)
    run = GOLDEN_RUNS[k]
    ctx = N.default_ctx()
    put = (lambda a: ctx.to_device(np.ascontiguousarray(a))) if resident else (lambda a: np.ascontiguousarray(a))
    image = Image(mat=put(run['page']))
    masks = [Mask(mat=put(r['mask']), box=Box(up=r['box'][0], down=r['box'][1], left=r['box'][2], right=r['box'][3]))
             for r in run['regions']]
    grouped = [[Polygon.from_smooth_xy(np.ascontiguousarray(q[:, ::-1], dtype=np.float32)) for q in r['chars']] for r in run['regions']]
    angles = [r['angle'] for r in run['regions']]
    with N.resident(resident):
        built = TextRegionFlattener.build_flattened_text_regions(image, [None] * run['n'], masks, run['typical'], angles, grouped)
        assert len(built) == run['n']
        for got, want in zip(built, run['built']):
            _region_equal(got, want, resident)
        same(built[0].text_region_image.mat, run['text_region_image0'])
        kept = [built[i] for i in run['keep']]
        resized = resize_flattened_text_regions(kept, [tuple(t) for t in run['targets']])
        for got, want in zip(resized, run['resized']):
            _region_equal(got, want, resident)
        if kept:
            _region_equal(kept[0].to_resized_flattened_text_region(*run['targets'][0]), run['resized'][0], resident)
        rotated = post_rotate_flattened_text_regions(resized, run['post'])
        for got, want, mid, angle in zip(rotated, run['rotated'], resized, run['post']):
            if angle == 0:
                assert got is mid
            else:
                _region_equal(got, want, resident)
        single = [i for i, a in enumerate(run['post']) if a]
        if single:
            _region_equal(resized[single[0]].to_post_rotated_flattened_text_region(run['post'][single[0]]),
                          run['rotated'][single[0]], resident)
        if not rotated:
            return
        stack = run['stack']
        got = stack_flattened_text_regions(stack['page_pad'], stack['pad'], rotated, lambda: R.ReplayPacker(stack['placements']))
        assert isinstance(got[0].arr, N.DevArray) == resident
        same(got[0].mat, stack['image'])
        same(got[1].mat, stack['mask'])
        assert [[b.up, b.down, b.left, b.right] for b in got[2]] == stack['boxes']
        _chars_equal(got[3], stack['chars'])
        assert list(got[4]) == stack['char_box_indices']


def test_background_matches_the_golden():
    from vkit_amd import _native as N
    from vkit_amd.pipeline.text_detection import build_background_image_for_stacking
    same(build_background_image_for_stacking(7, 11).mat, GOLDEN_BACKGROUND)
    with N.resident(True):
        image = build_background_image_for_stacking(7, 11)
        assert isinstance(image.arr, N.DevArray)
        same(image.mat, GOLDEN_BACKGROUND)
