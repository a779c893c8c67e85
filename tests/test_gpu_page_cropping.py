"""GPU: PageCroppingStep / Cropper on the MI355X (csrc/crop.hip) against the reference's own run (tests/golden/page_cropping.npz)
and the numpy restatement (tests/crop_restate.py)."""
import ctypes
import os
import sys
import time

import numpy as np
import pytest
from numpy.random import default_rng

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crop_restate as R  # noqa: E402
import cropping_fixture as F  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = F.cases()
IDS = [f"{c['name']}-{c['seed']}" for c in CASES]
INTER_AREA = 3


def _page(planes, is_prob, device):
    from vkit_amd import _native as N
    from vkit_amd.element import Image, Mask, ScoreMap
    from vkit_amd.pipeline.text_detection import PageResizingStepOutput
    ctx = N.default_ctx()
    held = {n: (ctx.to_device(p) if device else p) for n, p in planes.items()}
    return PageResizingStepOutput(
        page_image=Image(mat=held['page_image']),
        **{n: (ScoreMap(mat=held[n], is_prob=is_prob[n]) if planes[n].dtype == np.float32 else Mask(mat=held[n]))
           for n in R.PLANES[1:]})


def _run(planes, config, rng, is_prob, device):
    from vkit_amd.pipeline.text_detection import PageCroppingStep, PageCroppingStepInput
    return PageCroppingStep(config).run(PageCroppingStepInput(page_resizing_step_output=_page(planes, is_prob, device)), rng)


def _assert_pages_equal(got, want, device):
    """CroppedPage list vs restatement / fixture dicts, bit for bit."""
    assert len(got) == len(want)
    for page, w in zip(got, want):
        box = w['state'].target_core_box if 'state' in w else None
        assert F.box4(page.target_core_box) == (F.box4(box) if box is not None else list(w['target_core_box']))
        assert page.page_image.on_device == device
        assert np.array_equal(page.page_image.mat, w['page_image'])
        for name in R.LABELS:
            element = getattr(page, name)
            assert element.box == page.target_core_box
            assert element.mat.dtype == w[name].dtype and element.mat.tobytes() == w[name].tobytes(), name
        if 'down_page_char_mask' not in w:
            assert page.downsampled_label is None
            continue
        d = page.downsampled_label
        if 'down_shape' in w:
            assert d.shape == w['down_shape'] and F.box4(d.target_core_box) == list(w['down_target_core_box'])
        for name in R.LABELS:
            element = getattr(d, name)
            assert element.box is None
            assert element.mat.dtype == w['down_' + name].dtype and element.mat.tobytes() == w['down_' + name].tobytes(), name


@pytest.mark.parametrize('device', [False, True], ids=['host', 'device'])
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_run_equals_the_reference(case, device):
    from vkit_amd.pipeline.text_detection import PageCroppingStepConfig
    rng = default_rng(case['seed'])
    out = _run(case['planes'], PageCroppingStepConfig(**case['overrides']), rng, F.is_prob_of(case), device)
    _assert_pages_equal(out.cropped_pages, case['samples'], device)
    assert rng.bit_generator.state == case['rng_state']


@pytest.mark.parametrize('device', [False, True], ids=['host', 'device'])
def test_cropper_single_planes(device):
    from vkit_amd import _native as N
    from vkit_amd.element import Image, Mask, ScoreMap
    from vkit_amd.mechanism.cropper import Cropper
    rng = default_rng(7)
    ctx = N.default_ctx()
    for shape, core, pad in [((50, 70), 32, 8), ((20, 90), 32, 8), ((48, 48), 32, 8), ((10, 12), 16, 4)]:
        cropper = Cropper.create_from_random_proposal(shape=shape, core_size=core, pad_size=pad, rng=rng, pad_value=200)
        image = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
        gray = rng.integers(0, 256, shape, dtype=np.uint8)
        mask = (rng.random(shape) < 0.3).astype(np.uint8)
        score = rng.random(shape, dtype=np.float32)
        up = (lambda a: ctx.to_device(a)) if device else (lambda a: a)
        got = cropper.crop_image(Image(mat=up(image)))
        assert got.on_device == device and np.array_equal(got.mat, R.crop(image, cropper.cropper_state, fill=200))
        got = cropper.crop_image(Image(mat=up(gray)))
        assert np.array_equal(got.mat, R.crop(gray, cropper.cropper_state, fill=200))
        for core_only in (False, True):
            m = cropper.crop_mask(Mask(mat=up(mask)), core_only=core_only)
            assert np.array_equal(m.mat, R.crop(mask, cropper.cropper_state, core_only=core_only))
            assert m.box == (cropper.target_core_box if core_only else None)
            s = cropper.crop_score_map(ScoreMap(mat=up(score), is_prob=True), core_only=core_only)
            assert s.is_prob and s.mat.tobytes() == R.crop(score, cropper.cropper_state, core_only=core_only).tobytes()
            assert s.box == (cropper.target_core_box if core_only else None)


@pytest.mark.parametrize('factor', [2, 4])
def test_downsampled_planes_equal_the_resize_kernel(factor):
    """The shrink inside k_crop_planes is the INTER_AREA path of vkx_resize_* on the cropped core."""
    from vkit_amd import _native as N
    from vkit_amd.pipeline.text_detection import PageCroppingStepConfig
    rng = default_rng(factor)
    planes = dict(page_image=rng.integers(1, 256, (120, 100, 3), dtype=np.uint8),
                  page_active_mask=np.ones((120, 100), np.uint8),
                  page_char_mask=(rng.random((120, 100)) < 0.4).astype(np.uint8),
                  page_seal_impression_char_mask=(rng.random((120, 100)) < 0.1).astype(np.uint8),
                  page_char_height_score_map=rng.random((120, 100), dtype=np.float32),
                  page_text_line_mask=(rng.random((120, 100)) < 0.2).astype(np.uint8),
                  page_text_line_height_score_map=(rng.random((120, 100), dtype=np.float32) * 9).astype(np.float32))
    is_prob = {n: n == 'page_char_height_score_map' for n in R.LABELS}
    config = PageCroppingStepConfig(core_size=48, pad_size=8, downsample_labeling_factor=factor, num_samples=4,
                                    text_ratio_min=0.0, active_region_ratio_min=0.0)
    out = _run(planes, config, default_rng(3), is_prob, True)
    assert len(out.cropped_pages) == 4
    small = (48 // factor, 48 // factor)
    for page in out.cropped_pages:
        for name in R.LABELS:
            core = getattr(page, name).mat
            got = getattr(page.downsampled_label, name).mat
            if core.dtype == np.uint8:
                want = N.host_array(N.resize(((core > 0) * 255).astype(np.uint8), small, INTER_AREA)) > 0
            else:
                want = N.host_array(N.resize(core, small, INTER_AREA))
                if is_prob[name]:
                    want = np.clip(want, 0.0, 1.0)
            assert got.tobytes() == np.asarray(want, got.dtype).tobytes(), name


def test_chained_page_steps_equal_the_restatement():
    from vkit_amd.pipeline import text_detection as T
    from vkit_amd.pipeline.text_detection.synthetic_page import synthetic_page_input
    step_input = synthetic_page_input(seed=5, size=256, n_lines=24)
    rng = default_rng(11)
    a = T.page_assembler_step_factory.create().run(step_input, rng)
    d = T.page_distortion_step_factory.create().run(T.PageDistortionStepInput(a), rng)
    r = T.page_resizing_step_factory.create().run(T.PageResizingStepInput(d), rng)
    config = T.PageCroppingStepConfig(core_size=64, pad_size=16, text_ratio_min=0.005, active_region_ratio_min=0.2)
    planes = {n: np.array(getattr(r, n).mat) for n in R.PLANES}
    is_prob = {n: bool(getattr(r, n).is_prob) if planes[n].dtype == np.float32 else False for n in R.LABELS}
    mirror = default_rng(0)
    mirror.bit_generator.state = rng.bit_generator.state
    got = T.page_cropping_step_factory.create(config).run(T.PageCroppingStepInput(page_resizing_step_output=r), rng)
    want = R.run(planes, config, mirror, is_prob)
    assert rng.bit_generator.state == mirror.bit_generator.state
    _assert_pages_equal(got.cropped_pages, want, r.page_image.on_device)


def test_device_run_launches_and_syncs():
    """A device-resident page: the crop path is at most two launches (the context's timing table)."""
    from vkit_amd import _native as N
    from vkit_amd.pipeline.text_detection import PageCroppingStepConfig
    case = next(c for c in CASES if c['name'] == 'larger' and c['samples'])
    ctx = N.default_ctx()
    page = _page(case['planes'], F.is_prob_of(case), True)
    from vkit_amd.pipeline.text_detection import PageCroppingStep, PageCroppingStepInput
    step = PageCroppingStep(PageCroppingStepConfig(**case['overrides']))
    step.run(PageCroppingStepInput(page_resizing_step_output=page), default_rng(case['seed']))    # warm the scratch slots
    ctx.sync()
    ctx.set_timing(1)
    try:
        ctx.reset_timings()
        out = step.run(PageCroppingStepInput(page_resizing_step_output=page), default_rng(case['seed']))
        timings = ctx.timings()
    finally:
        ctx.set_timing(0)
    crop_launches = sum(n for name, (_ms, n) in timings.items() if name.startswith('k_crop'))
    assert out.cropped_pages and crop_launches <= 2, timings
    assert set(timings) <= {'k_crop_count', 'k_crop_planes'}, timings
    assert all(p.page_image.on_device for p in out.cropped_pages)


def _lib():
    from vkit_amd import _native as N
    return N, N.lib()


def test_abi_refusals_leave_canaries():
    N, L = _lib()
    ctx = N.default_ctx()
    h, w, core, pad = 40, 50, 16, 4
    crop = core + 2 * pad
    page = ctx.to_device(np.full((h, w), 1, np.uint8))
    image = ctx.to_device(np.full((h, w, 3), 9, np.uint8))
    canary = ctx.to_device(np.full((crop, crop), 0xAB, np.uint8))
    down = ctx.to_device(np.full((core // 2, core // 2), 0xAB, np.uint8))
    partials = ctx.to_device(np.full((2, 1, 2), -7, np.int64))
    good = (0, 0, crop, crop, 0, 0)

    def plane(**kw):
        rec = dict(src=page.ptr, dst=canary.ptr, dst_down=None, cn=1, is_f32=0, core_only=0, is_mask=1, clip=0, fill=0, window=0)
        rec.update(kw)
        table = (N.VkxCropPlane * 1)()
        for k, v in rec.items():
            setattr(table[0], k, v)
        return table

    def planes_call(windows=(good,), factor=0, **kw):
        return L.vkx_crop_planes_dev(ctx.handle, h, w, core, pad, factor, N._crop_window_table(windows), len(windows),
                                     plane(**kw), 1)

    def count_call(windows=(good,), img=image.ptr, cn=3, parts=1):
        return L.vkx_crop_count_dev(ctx.handle, ctypes.c_void_p(img) if img else None, h, w, cn, ctypes.c_void_p(page.ptr),
                                    ctypes.c_void_p(page.ptr), core, pad, N._crop_window_table(windows), len(windows), parts,
                                    ctypes.c_void_p(partials.ptr))

    refusals = [
        planes_call(src=None), planes_call(dst=None),
        planes_call(windows=((h - crop + 1, 0, crop, crop, 0, 0),)),          # past the page
        planes_call(windows=((-1, 0, crop, crop, 0, 0),)),
        planes_call(windows=((0, 0, crop, crop, 1, 0),)),                     # past the crop
        planes_call(windows=((0, 0, 0, crop, 0, 0),)),                        # empty
        planes_call(cn=2), planes_call(cn=3, is_f32=1),
        planes_call(window=1),
        planes_call(factor=3, core_only=1, dst_down=down.ptr),                 # does not divide
        planes_call(dst_down=down.ptr, core_only=1),                           # a shrink without a factor
        planes_call(dst=page.ptr + 8),                                          # overlaps the source
        planes_call(factor=2, core_only=1, dst_down=page.ptr),
        planes_call(fill=256),
        count_call(img=None, windows=((0, 0, crop, crop, 0, 1),)),
        count_call(cn=2),
        count_call(parts=0),
    ]
    assert refusals == [-1] * len(refusals), refusals      # VKX_ERR_INVALID
    ctx.sync()
    assert (canary.host() == 0xAB).all() and (down.host() == 0xAB).all() and (partials.host() == -7).all()
    # and a count whose partials overlap its source is refused too
    assert L.vkx_crop_count_dev(ctx.handle, None, h, w, 1, ctypes.c_void_p(page.ptr), ctypes.c_void_p(page.ptr), core, pad,
                                N._crop_window_table([good]), 1, 1, ctypes.c_void_p(page.ptr)) == -1
    assert (page.host() == 1).all()
    # the good calls run
    assert planes_call() == 0 and count_call() == 0
    ctx.sync()
    canary.invalidate_host()
    assert (canary.host() == 1).all()


def test_soak_random_configurations():
    """A few hundred random pages and configs against the restatement (fixed count, bounded time)."""
    from vkit_amd.pipeline.text_detection import PageCroppingStepConfig
    meta = default_rng(2026)
    start, n = time.monotonic(), 0
    while n < 300 and time.monotonic() - start < 120:
        factor = int(meta.choice([1, 2, 4]))
        core = factor * int(meta.integers(max(2, 8 // factor), 12))
        pad = factor * int(meta.integers(0, 5))
        h, w = (int(meta.integers(3, 2 * (core + 2 * pad))) for _ in range(2))
        active = np.zeros((h, w), np.uint8)
        y0, x0 = int(meta.integers(0, h)), int(meta.integers(0, w))
        active[y0:, x0:] = 1
        planes = dict(page_image=meta.integers(0, 3, (h, w, 3), dtype=np.uint8) * active[..., None],
                      page_active_mask=active, page_char_mask=(meta.random((h, w)) < meta.random()).astype(np.uint8),
                      page_seal_impression_char_mask=meta.integers(0, 3, (h, w), dtype=np.uint8),
                      page_char_height_score_map=meta.random((h, w), dtype=np.float32),
                      page_text_line_mask=(meta.random((h, w)) < 0.3).astype(np.uint8),
                      page_text_line_height_score_map=(meta.random((h, w), dtype=np.float32) * 30).astype(np.float32))
        is_prob = {name: name == 'page_char_height_score_map' for name in R.LABELS}
        num_samples = None if meta.random() < 0.5 else int(meta.integers(0, 6))
        config = PageCroppingStepConfig(
            core_size=core, pad_size=pad, num_samples=num_samples,
            num_samples_max=None if meta.random() < 0.5 else int(meta.integers(0, 5)),
            pad_value=int(meta.integers(0, 256)), text_ratio_min=float(meta.random() * 0.3),
            active_region_ratio_min=float(meta.random() * 0.8),
            drop_cropped_page_with_small_text_ratio=bool(meta.random() < 0.8),
            drop_cropped_page_with_small_active_region=bool(meta.random() < 0.8),
            enable_downsample_labeling=bool(meta.random() < 0.8) and factor > 1, downsample_labeling_factor=max(factor, 2))
        seed = int(meta.integers(0, 1 << 30))
        want_rng, got_rng = default_rng(seed), default_rng(seed)
        want = R.run(planes, config, want_rng, is_prob)
        got = _run(planes, config, got_rng, is_prob, bool(n % 2))
        _assert_pages_equal(got.cropped_pages, want, bool(n % 2))
        assert got_rng.bit_generator.state == want_rng.bit_generator.state
        n += 1
    assert n >= 100, n
