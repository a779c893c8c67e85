"""GPU: vkit_amd.torch_bridge on the MI355X -- zero-copy views in both directions, the ordering of the context's stream against
torch's, and the batch collate (csrc/collate.hip) against tests/collate_restate.py, bit for bit.  One process, one context."""
import ctypes
import os
import sys

import numpy as np
import pytest
from numpy.random import default_rng

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import collate_restate as R  # noqa: E402
from collate_gpu_cases import CANARY, LABELS, _carve, _mods, _samples  # noqa: E402

pytestmark = pytest.mark.gpu



def test_as_tensor_is_the_plane_itself():
    torch, N, TB = _mods()
    from vkit_amd.element import Image, Mask, ScoreMap
    ctx = N.default_ctx()
    rng = default_rng(1)
    image = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    score = rng.random((7, 5), dtype=np.float32)
    for element, want in ((Image(mat=ctx.to_device(image)), image), (Mask(mat=ctx.to_device(image[:, :, 0] & 1)), image[:, :, 0] & 1),
                          (ScoreMap(mat=ctx.to_device(score), is_prob=False), score)):
        t = TB.as_tensor(element)
        assert t.is_cuda and t.device.index == ctx.device and tuple(t.shape) == want.shape and t.data_ptr() == element.arr.ptr
        assert t.dtype == (torch.uint8 if want.dtype == np.uint8 else torch.float32)
        assert np.array_equal(t.cpu().numpy(), want) and np.array_equal(element.arr.host(), want)
    block = ctx.to_device(np.arange(64, dtype=np.uint8))
    view = N.DevView(block, 5, (3, 4, 3))
    t = TB.as_tensor(view)
    assert t.data_ptr() == block.ptr + 5 and np.array_equal(t.cpu().numpy(), np.arange(5, 41, dtype=np.uint8).reshape(3, 4, 3))
    assert block._viewed == {0} and view._viewed is block._viewed        # torch's default stream has handle 0
    # the tensor keeps the array alive: the block is not handed out again while the tensor lives
    ptr = block.ptr
    del view, block
    other = ctx.dev_empty((64,))
    assert other.ptr != ptr and int(t[0, 0, 0]) == 5


def test_writes_cross_the_streams_without_a_synchronise(monkeypatch):
    torch, N, TB = _mods()
    ctx = N.default_ctx()
    syncs = []
    real_sync = N.Context.sync
    monkeypatch.setattr(N.Context, 'sync', lambda self: syncs.append(1) or real_sync(self))
    rng = default_rng(2)
    host = rng.integers(0, 200, (16, 20, 3), dtype=np.uint8)
    lut = ((np.arange(256) * 7 + 3) % 256).astype(np.uint8)
    side = torch.cuda.Stream()
    arr = ctx.to_device(host)
    with torch.cuda.stream(side):
        t = TB.as_tensor(arr)
        for _ in range(20):                       # torch writes through the view on ITS stream ...
            t.add_(1)
            t.sub_(1)
        t.add_(5)
    assert arr._viewed == {int(side.cuda_stream)}
    got = N.apply_lut(arr, np.stack([lut] * 3))                # ... and the library's next read of the array waits for that stream
    assert not syncs
    assert np.array_equal(got.host(), lut[host + 5])
    # the other way round: the library writes, torch reads its result at once
    with torch.cuda.stream(side):
        blurred = N.gaussian_blur(arr, 5, 1.0)
        doubled = TB.as_tensor(blurred).to(torch.int32) * 2
    assert not syncs
    assert np.array_equal(doubled.cpu().numpy(), N.host_array(N.gaussian_blur(host + 5, 5, 1.0)).astype(np.int32) * 2)


def test_from_tensor_through_rotate():
    torch, N, TB = _mods()
    from vkit_amd.element import Image
    from vkit_amd.mechanism.distortion import rotate
    ctx = N.default_ctx()
    host = default_rng(3).integers(0, 256, (16, 20, 3), dtype=np.uint8)
    t = torch.from_numpy(host).to(f'cuda:{ctx.device}')
    arr = TB.from_tensor(t)
    assert arr.ptr == t.data_ptr() and arr.shape == (16, 20, 3) and arr.tensor is t and arr.ctx is ctx
    got = rotate.distort_image({'angle': 30}, Image(mat=arr))
    want = rotate.distort_image({'angle': 30}, Image(mat=host))
    assert got.on_device and got.shape == want.shape and np.array_equal(got.mat, want.mat)
    TB.release(arr)
    assert np.array_equal(t.cpu().numpy(), host)
    f = torch.arange(12, dtype=torch.float32, device=t.device).reshape(3, 4)
    assert np.array_equal(TB.from_tensor(f).host(), np.arange(12, dtype=np.float32).reshape(3, 4))
    with pytest.raises(ValueError, match='contiguous'):
        TB.from_tensor(f.t())
    with pytest.raises(TypeError, match='uint8 or float32'):
        TB.from_tensor(f.to(torch.float16))


def test_external_ordering_entry_points():
    torch, N, TB = _mods()
    ctx = N.default_ctx()
    L = N.lib()
    side = torch.cuda.Stream()
    for stream in (0, int(side.cuda_stream), int(L.vkx_ctx_stream(ctx.handle))):
        ctx.wait_external(stream)
        ctx.signal_external(stream)
    assert L.vkx_ctx_wait_external(None, None) == -1 and L.vkx_ctx_signal_external(None, None) == -1
    ctx.sync()
    torch.cuda.synchronize()


# ---- the collate -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('channels_first', [True, False], ids=['nchw', 'nhwc'])
@pytest.mark.parametrize('dtype', R.DTYPES)
@pytest.mark.parametrize('shape,label_shape', [((5, 5), (3, 5)), ((8, 12), (4, 4)), ((7, 9), (4, 8))], ids=['5x5', '8x12', '7x9'])
@pytest.mark.parametrize('n', [1, 3])
def test_collate_equals_the_restatement(n, shape, label_shape, dtype, channels_first):
    """Sources at byte offsets 0 .. 3; label planes of 15 / 16 / 32 bytes (uint8) and 60 / 64 / 128 bytes (float32), their shrunk
    forms smaller still; fresh outputs, then ``out=`` tensors between canaries."""
    torch, N, TB = _mods()
    ctx = N.default_ctx()
    rng = default_rng(100 * n + shape[0])
    for first_offset in range(4):
        samples, host = _samples(N, ctx, rng, n, shape, label_shape, first_offset)
        want = {'page_image': R.collate_images(host['page_image'], dtype, channels_first=channels_first)}
        want.update({key: R.collate_planes(planes) for key, planes in host.items() if key != 'page_image'})
        got = TB.collate_cropped_pages(samples, image_dtype=dtype, channels_first=channels_first)
        assert set(got) == set(want) | {'target_core_box', 'downsampled_target_core_box'}
        device = got['page_image'].device
        wanted = {key: (tuple(got[key].shape), got[key].dtype) for key in want}
        buffer, out, used = _carve(torch, device, wanted)
        again = TB.collate_cropped_pages(samples, image_dtype=dtype, channels_first=channels_first, out=out)
        for key, w in want.items():
            assert got[key].is_cuda and got[key].is_contiguous() and tuple(got[key].shape) == tuple(w.shape), key
            assert got[key].dtype == getattr(torch, dtype) if key == 'page_image' else str(got[key].dtype) == 'torch.' + str(w.dtype), key
            assert R.same_bits(got[key], w), (key, first_offset)
            assert again[key] is out[key] and R.same_bits(again[key], w), (key, first_offset)
        assert (buffer.cpu().numpy()[~used] == CANARY).all(), 'a byte outside the outputs was written'
        assert got['target_core_box'].dtype == torch.int32 and not got['target_core_box'].is_cuda
        assert got['target_core_box'].tolist() == [[2 + i, 5, 3, 6 + i] for i in range(n)]
        assert got['downsampled_target_core_box'].tolist() == [[i, i + 1, 1, 2] for i in range(n)]


def test_collate_without_downsampled_and_text_regions():
    torch, N, TB = _mods()
    from vkit_amd.element import Box, Image, Mask, ScoreMap
    from vkit_amd.pipeline.text_detection.page_text_region_cropping import CroppedPageTextRegion
    ctx = N.default_ctx()
    rng = default_rng(9)
    samples, host = _samples(N, ctx, rng, 2, (6, 7), (3, 3), 1)
    got = TB.collate_cropped_pages(samples, image_dtype=torch.float16, downsampled=False)
    assert not any(key.startswith('downsampled_') for key in got) and len(got) == 1 + len(LABELS) + 1
    assert R.same_bits(got['page_image'], R.collate_images(host['page_image'], 'float16'))
    with pytest.raises(ValueError, match='out'):
        TB.collate_cropped_pages(samples, image_dtype=torch.float32, downsampled=False, out=got)     # float16 from the call before

    regions, planes = [], {}
    for i in range(2):
        mats = dict(page_image=rng.integers(0, 256, (6, 10, 3), dtype=np.uint8), page_char_mask=rng.integers(0, 2, (4, 5), dtype=np.uint8),
                    page_char_height_score_map=rng.random((4, 5), dtype=np.float32), page_char_gaussian_score_map=rng.random((4, 5), dtype=np.float32),
                    page_char_bounding_box_mask=rng.integers(0, 2, (4, 5), dtype=np.uint8))
        for key, m in mats.items():
            planes.setdefault(key, []).append(m)
        held = {key: ctx.to_device(m) for key, m in mats.items()}
        regions.append(CroppedPageTextRegion(
            page_image=Image(mat=held['page_image']), page_char_mask=Mask(mat=held['page_char_mask']),
            page_char_height_score_map=ScoreMap(mat=held['page_char_height_score_map'], is_prob=False),
            page_char_gaussian_score_map=ScoreMap(mat=held['page_char_gaussian_score_map'], is_prob=False),
            page_char_regression_labels=[('label', i)], page_char_bounding_box_mask=Mask(mat=held['page_char_bounding_box_mask']),
            target_core_box=Box(up=1, down=4, left=1, right=5), downsampled_label=None))
    got = TB.collate_cropped_page_text_regions(regions, image_dtype='bfloat16', channels_first=False, downsampled=False)
    assert R.same_bits(got['page_image'], R.collate_images(planes['page_image'], 'bfloat16', channels_first=False))
    for key in planes:
        if key != 'page_image':
            assert R.same_bits(got[key], R.collate_planes(planes[key])), key
    assert got['page_char_regression_labels'] == [[('label', 0)], [('label', 1)]]
    with pytest.raises(ValueError, match='downsampled_label'):
        TB.collate_cropped_page_text_regions(regions)


def _cropped_pages(N, seed=4):
    from vkit_amd.element import Image, Mask, ScoreMap
    from vkit_amd.pipeline.text_detection import (PageCroppingStep, PageCroppingStepConfig, PageCroppingStepInput,
                                                  PageResizingStepOutput)
    rng = default_rng(seed)
    shape = (64, 96)
    planes = dict(page_image=rng.integers(1, 256, shape + (3,), dtype=np.uint8), page_active_mask=np.ones(shape, np.uint8),
                  page_char_mask=(rng.random(shape) < 0.4).astype(np.uint8),
                  page_seal_impression_char_mask=(rng.random(shape) < 0.1).astype(np.uint8),
                  page_char_height_score_map=rng.random(shape, dtype=np.float32),
                  page_text_line_mask=(rng.random(shape) < 0.2).astype(np.uint8),
                  page_text_line_height_score_map=(rng.random(shape, dtype=np.float32) * 9).astype(np.float32))
    config = PageCroppingStepConfig(core_size=16, pad_size=4, num_samples=3, text_ratio_min=0.0, active_region_ratio_min=0.0)
    ctx = N.default_ctx()
    with N.resident(True):
        held = {k: ctx.to_device(p) for k, p in planes.items()}
        page = PageResizingStepOutput(
            page_image=Image(mat=held['page_image']),
            **{k: (ScoreMap(mat=held[k], is_prob=k == 'page_char_height_score_map') if p.dtype == np.float32 else Mask(mat=held[k]))
               for k, p in planes.items() if k != 'page_image'})
        out = PageCroppingStep(config).run(PageCroppingStepInput(page_resizing_step_output=page), default_rng(seed))
    assert len(out.cropped_pages) == 3 and all(p.page_image.on_device for p in out.cropped_pages)
    return out.cropped_pages


def test_page_cropping_step_into_a_batch():
    torch, N, TB = _mods()
    pages = _cropped_pages(N)
    batch = TB.collate_cropped_pages(pages)
    assert tuple(batch['page_image'].shape) == (3, 3, 24, 24) and batch['page_image'].dtype == torch.float32
    assert R.same_bits(batch['page_image'], R.collate_images([p.page_image.mat for p in pages]))
    for name in LABELS:
        assert tuple(batch[name].shape) == (3, 16, 16) and tuple(batch['downsampled_' + name].shape) == (3, 8, 8)
        assert R.same_bits(batch[name], R.collate_planes([getattr(p, name).mat for p in pages])), name
        assert R.same_bits(batch['downsampled_' + name], R.collate_planes([getattr(p.downsampled_label, name).mat for p in pages])), name
    assert batch['target_core_box'].tolist() == [[4, 19, 4, 19]] * 3 and batch['downsampled_target_core_box'].tolist() == [[2, 9, 2, 9]] * 3
    # the caller may use the tensors and drop the samples at once
    del pages
    total = float(batch['page_image'].sum()) + float(batch['page_char_mask'].sum())
    assert np.isfinite(total)


def test_collate_launches_and_syncs(monkeypatch):
    torch, N, TB = _mods()
    ctx = N.default_ctx()
    pages = _cropped_pages(N, seed=6)
    out = TB.collate_cropped_pages(pages, image_dtype='bfloat16')                 # warm the scratch slot and torch's allocator
    ctx.sync()
    syncs = []
    real_sync = N.Context.sync
    monkeypatch.setattr(N.Context, 'sync', lambda self: syncs.append(1) or real_sync(self))
    ctx.set_timing(1)
    try:
        ctx.reset_timings()
        del syncs[:]
        TB.collate_cropped_pages(pages, image_dtype='bfloat16', out=out)
        n_syncs = len(syncs)
        timings = ctx.timings()
    finally:
        ctx.set_timing(0)
    assert n_syncs == 0
    assert set(timings) == {'k_collate_images', 'k_collate_planes'}, timings
    assert sum(n for name, (_ms, n) in timings.items() if name.startswith('k_collate')) <= 2, timings


def test_collate_abi_refusals_leave_canaries():
    torch, N, TB = _mods()
    L = N.lib()
    ctx = N.default_ctx()
    h, w = 6, 8
    src = ctx.to_device(np.full((h, w, 3), 7, np.uint8))
    plane_src = ctx.to_device(np.full((64,), 3, np.uint8))
    batch = ctx.to_device(np.full((h * w * 3 * 4 + 64,), CANARY, np.uint8))
    plane_dst = ctx.to_device(np.full((128,), CANARY, np.uint8))

    def call(images=(src.ptr,), n_images=None, planes=((plane_src.ptr, plane_dst.ptr, 64),), n_planes=None, norm=True, **kw):
        image_table = (N.VkxCollateImage * max(1, len(images)))()
        for rec, p in zip(image_table, images):
            rec.src = p
        plane_table = (N.VkxCollatePlane * max(1, len(planes)))()
        for rec, (s, d, b) in zip(plane_table, planes):
            rec.src, rec.dst, rec.bytes = s, d, b
        mean, scale = kw.pop('mean_', (1.0, 2.0, 3.0)), kw.pop('scale_', (0.5, 0.25, 0.125))
        rec = dict(dst=batch.ptr, height=h, width=w, dtype=TB.COLLATE_F32, channels_first=1)
        rec.update(kw)
        nrm = N.VkxCollateNorm()
        for k, v in rec.items():
            setattr(nrm, k, v)
        nrm.mean[:], nrm.scale[:] = mean, scale
        return L.vkx_collate_dev(ctx.handle, image_table if images is not None and len(images) else None,
                                 len(images) if n_images is None else n_images, plane_table if len(planes) else None,
                                 len(planes) if n_planes is None else n_planes, ctypes.byref(nrm) if norm else None)

    refusals = [
        call(images=(), n_images=1),                                      # NULL tables with non-zero counts
        call(planes=(), n_planes=1),
        call(norm=False),
        call(height=0), call(width=0), call(width=32769),                 # a zero side
        call(dst=src.ptr + 16),                                           # the batch overlaps a source
        call(planes=((plane_src.ptr, plane_src.ptr + 32, 64),)),          # a plane overlaps its source
        call(planes=((plane_src.ptr, src.ptr + 8, 16),)),                 # a plane lands in an image source
        call(planes=((plane_src.ptr, plane_dst.ptr, 64), (plane_src.ptr, plane_dst.ptr + 63, 8))),   # two destinations overlap
        call(planes=((plane_src.ptr, batch.ptr + 8, 16),)),               # a plane lands in the image batch
        call(dtype=4), call(dtype=-1),                                    # an unknown dtype code
        call(channels_first=2),
        call(dst=batch.ptr + 2),                                          # float32 at an odd address
        call(images=(None,)), call(dst=None),
        call(planes=((plane_src.ptr, plane_dst.ptr, 0),)), call(planes=((None, plane_dst.ptr, 8),)),
        call(n_images=-1), call(n_planes=-1), call(n_images=65536),
        call(mean_=(float('nan'), 0.0, 0.0)), call(scale_=(1.0, float('inf'), 1.0)),
        L.vkx_collate_dev(None, None, 0, None, 0, None),
    ]
    assert refusals == [-1] * len(refusals), (refusals, N.last_error())      # VKX_ERR_INVALID
    ctx.sync()
    assert (batch.host() == CANARY).all() and (plane_dst.host() == CANARY).all()
    assert (src.host() == 7).all() and (plane_src.host() == 3).all()
    # nothing to do is fine, and the good call runs
    assert L.vkx_collate_dev(ctx.handle, None, 0, None, 0, None) == 0
    assert call() == 0
    ctx.sync()
    batch.invalidate_host()
    plane_dst.invalidate_host()
    got = batch.host()
    want = R.bits(np.ascontiguousarray(np.broadcast_to(((np.float32(7) - np.array([1, 2, 3], np.float32)) *
                                                        np.array([0.5, 0.25, 0.125], np.float32))[:, None, None], (3, h, w))))
    assert np.array_equal(got[:h * w * 12].view(np.uint32).reshape(3, h, w), want) and (got[h * w * 12:] == CANARY).all()
    assert (plane_dst.host()[:64] == 3).all() and (plane_dst.host()[64:] == CANARY).all()
