"""jpeg_quality on the device (csrc/jpeg.hip, vkx_jpeg_roundtrip_u8[_dev]): bit for bit the libjpeg-turbo round trip of
cv.imencode / cv.imdecode (photometric/effect.py:41-42), against tests/golden/jpeg_roundtrip.npz and tests/jpeg_restate.py,
through the wrapper, the operator under out_of_path='device', RandomDistortion and PageDistortionStep."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
from numpy.random import default_rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import jpeg_restate as J  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def N():
    from vkit_amd import _native
    return _native


def golden_cases(golden_dir):
    z = np.load(os.path.join(golden_dir, 'jpeg_roundtrip.npz'))
    for i, name in enumerate(z['names']):
        yield str(name), z[f'in_{i}'], z[f'q_{i}'], z[f'out_{i}']


def test_every_golden_case_from_host_and_device_arrays(N, golden_dir):
    ctx = N.default_ctx()
    for name, mat, qualities, outs in golden_cases(golden_dir):
        dev = ctx.to_device(np.ascontiguousarray(mat))
        for q, want in zip(qualities, outs):
            got = N.jpeg_roundtrip(mat, int(q))
            assert isinstance(got, np.ndarray) and got.shape == want.shape
            assert (got == want).all(), (name, int(q), 'host')
            got_dev = N.jpeg_roundtrip(dev, int(q))
            assert isinstance(got_dev, N.DevArray)
            assert (got_dev.host() == want).all(), (name, int(q), 'device')


def test_operator_under_out_of_path_device_gives_the_goldens(N, golden_dir):
    from vkit_amd.element import Image
    from vkit_amd.mechanism.distortion.photometric.effect import jpeg_quality, JpegQualityConfig
    from vkit_amd.mechanism.distortion.photometric.opt import out_of_path
    for name, mat, qualities, outs in golden_cases(golden_dir):
        if max(mat.shape[:2]) > 300:
            continue
        for q, want in list(zip(qualities, outs))[::3]:
            with out_of_path('device'):
                res = jpeg_quality.distort(JpegQualityConfig(quality=int(q)), image=Image(mat=mat))
            assert (res.image.mat == want).all(), (name, int(q))
            assert 'out_of_path' not in (res.meta or {})
    # the default stays the pass-through
    mat = next(golden_cases(golden_dir))[1]
    res = jpeg_quality.distort(JpegQualityConfig(quality=10), image=Image(mat=mat))
    assert (res.image.mat == mat).all() and res.meta == {'out_of_path': ('jpeg_quality',)}


def test_random_distortion_device_mode_follows_the_reference_stream(N, golden_dir):
    from vkit_amd.element import Image
    from vkit_amd.mechanism.distortion_policy import random_distortion_factory
    from vkit_amd.mechanism.distortion_policy.random_distortion import RandomDistortionDebug
    with open(os.path.join(golden_dir, 'policy_configs.json')) as f:
        records = [r for r in json.load(f) if r['name'] == 'jpeg_quality']
    assert records
    rd = random_distortion_factory.create(None, out_of_path='device')
    policy = [p for p in rd.stages[0].config.distortion_policies if p.name == 'jpeg_quality'][0]
    for rec in records:
        image = Image(mat=default_rng(rec['seed']).integers(0, 256, tuple(rec['shape']) + (3,), dtype=np.uint8))
        rng = default_rng(rec['seed'])
        from vkit_amd.mechanism.distortion.photometric.opt import out_of_path
        with out_of_path('device'):
            res = policy.distort(level=rec['level'], image=image, rng=rng, enable_debug=True)
        assert res.config.quality == rec['config']['quality']
        assert float(rng.random()) == rec['next_random']          # exactly the reference's draws
        assert (res.image.mat == J.jpeg_roundtrip(image.mat, rec['config']['quality'])).all()
        assert 'out_of_path' not in (res.meta or {})

    # a RandomDistortion restricted to jpeg_quality (test_host_golden.py's table), the switch on the factory
    others = [f.name for f in random_distortion_factory.photometric_policy_factories if f.name != 'jpeg_quality']
    config = {'prob_photometric': 1.0, 'num_photometric_min': 1, 'num_photometric_max': 1, 'prob_geometric': 0.0,
              'disabled_policy_names': others}
    image = Image(mat=default_rng(0).integers(0, 256, (96, 80, 3), dtype=np.uint8))
    changed = 0
    for seed in range(8):
        debug = RandomDistortionDebug()
        out = random_distortion_factory.create(config, out_of_path='device').distort(default_rng(seed), image=image, debug=debug)
        assert debug.distortion_names == ['jpeg_quality']
        q = debug.distortion_configs[0].quality
        assert (out.image.mat == J.jpeg_roundtrip(image.mat, q)).all(), seed
        assert 'out_of_path' not in (out.meta or {})
        # the same draws as the pass-through run: only the image differs
        passed = random_distortion_factory.create(config).distort(default_rng(seed), image=image)
        assert passed.meta == {'out_of_path': ('jpeg_quality',)}
        changed += int((out.image.mat != image.mat).any())
    assert changed == 8


def test_soak_random_shapes_qualities_modes_and_rois(N):
    """~2000 seeded cases, shapes log-uniform up to 1024 per side, every quality, RGB and grayscale; a quarter of them read a
    region of interest of a larger plane (row stride > row bytes) through the C entry points, on the host and the device."""
    ctx = N.default_ctx()
    lib = N.lib()
    rng = default_rng(2026)
    for i in range(2000):
        h, w = (int(v) for v in np.exp(rng.uniform(0, np.log(1024), 2)))
        q = int(rng.integers(0, 101))
        cn = 1 if rng.random() < 0.3 else 3
        shape = (h, w) if cn == 1 else (h, w, 3)
        if i % 3 == 0:
            mat = rng.integers(0, 256, shape, dtype=np.uint8)
        elif i % 3 == 1:
            mat = (rng.integers(0, 2, shape) * 255).astype(np.uint8)
        else:           # smooth ramps, a different slope per channel
            ramp = np.add.outer(np.arange(h), np.arange(w))[..., None] * np.array([1, 3, 7][:cn])
            mat = np.ascontiguousarray((ramp % 256).astype(np.uint8).reshape(shape))
        want = J.jpeg_roundtrip(mat, q)
        if i % 4 != 3:
            got = N.jpeg_roundtrip(mat if i % 2 else ctx.to_device(mat), q)
            got = got.host() if isinstance(got, N.DevArray) else got
            assert (got == want).all(), (i, shape, q)
            continue
        # ROI: the image sits at (3, 5) inside a larger plane; the destination has a stride of its own too
        big = rng.integers(0, 256, (h + 7, w + 9) + shape[2:], dtype=np.uint8)
        big[3:3 + h, 5:5 + w] = mat
        row = (w + 9) * cn
        dst_stride = (w + 3) * cn
        off = 3 * row + 5 * cn
        if i % 8 == 3:      # host pointers
            dst = np.zeros((h, w + 3) + shape[2:], np.uint8)
            N.check(lib.vkx_jpeg_roundtrip_u8(ctx.handle, ctypes.c_void_p(big.ctypes.data + off), h, w, cn, row,
                                              ctypes.c_void_p(dst.ctypes.data), dst_stride, q))
            got = dst[:, :w]
        else:               # device pointers
            dbig = ctx.to_device(big)
            ddst = ctx.dev_empty((h, w + 3) + shape[2:], np.uint8)
            N.check(lib.vkx_jpeg_roundtrip_u8_dev(ctx.handle, ctypes.c_void_p(dbig.ptr + off), h, w, cn, row,
                                                  ctypes.c_void_p(ddst.ptr), dst_stride, q))
            ctx.sync()
            ddst.invalidate_host()
            got = ddst.host()[:, :w]
        assert (got == want).all(), (i, shape, q, 'roi')


def test_page_distortion_step_under_env_device(N, monkeypatch):
    from vkit_amd.element import Mask
    from vkit_amd.mechanism.distortion_policy import random_distortion_factory
    from vkit_amd.mechanism.distortion_policy.random_distortion import RandomDistortionDebug
    from vkit_amd.pipeline import text_detection as T
    from vkit_amd.pipeline.text_detection.synthetic_page import synthetic_page_input
    page_output = T.page_assembler_step_factory.create().run(synthetic_page_input(seed=9, size=256, n_lines=24), default_rng(0))
    others = [f.name for f in random_distortion_factory.photometric_policy_factories if f.name != 'jpeg_quality']
    factory_config = {'prob_photometric': 1.0, 'num_photometric_min': 1, 'num_photometric_max': 1, 'prob_geometric': 0.0,
                      'disabled_policy_names': others}
    monkeypatch.setenv('VKX_OUT_OF_PATH', 'device')
    step = T.page_distortion_step_factory.create({'random_distortion_factory_config': factory_config})
    seed = 4
    out = step.run(T.PageDistortionStepInput(page_output), default_rng(seed))
    page_image = np.asarray(page_output.page.image.mat)
    # the quality the step drew: the same chain driven directly on the same stream
    debug = RandomDistortionDebug()
    random_distortion_factory.create(factory_config).distort(
        image=page_output.page.image, mask=Mask(mat=np.ones(page_image.shape[:2], np.uint8)), rng=default_rng(seed), debug=debug)
    assert debug.distortion_names == ['jpeg_quality']
    want = J.jpeg_roundtrip(page_image, debug.distortion_configs[0].quality)
    got = np.asarray(out.page_image.mat)
    active = np.asarray(out.page_active_mask.mat) > 0
    assert active.sum() > 0.9 * active.size
    assert (got != page_image).any()
    assert (got[active] == want[active]).all()
