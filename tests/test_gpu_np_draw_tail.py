"""The ziggurat tail of the integer kinds, decided from float32 logarithm estimates (nprand.hip: kTailEps, tail_log_est), against
numpy ITSELF: every int16, the draws consumed and the generator state, over enough samples to hold 10^5 tail events, with and
without VKX_NP_DEBUG_WIDE_MARGIN (which puts every tail pass through the float64 log1p); and the estimate against float64 log1p.
Every figure is printed before it is asserted (pytest -s shows them)."""
import ctypes
import os
import re

import numpy as np
import pytest

from vkit_amd import _native as N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE_MARGIN = 0x100     # VKX_NP_DEBUG_WIDE_MARGIN
AMBIGUOUS, SHORT = 1, 2

# (seed, std): 20 streams of 26 000 000 samples = 5.2e8.  The proof of an emitted integer scales with std: the bench's 10, small ones
# (0.5 and 1: nearly every tail sample far from a half-integer), large ones (50 .. 399: the window a thousand times wider)
SAMPLES = 26_000_000
STREAMS = [(1000 + k, std) for k, std in enumerate([10.0, 0.5, 1.0, 50.0, 399.0, 10.0, 2.5, 120.0, 37.0, 10.0,
                                                     64.0, 0.9, 255.0, 10.0, 7.25, 80.0, 10.0, 199.5, 3.0, 10.0])]
assert len(STREAMS) * SAMPLES >= 5e8


def _ki0():
    text = open(os.path.join(ROOT, 'vkit_amd', 'csrc', 'np_ziggurat.h')).read()
    body = re.search(r'kNpZigK\[256\]\s*=\s*\{(.*?)\}', text, re.S).group(1)
    return np.uint64(int(body.split(',')[0].strip().rstrip('uUlL'), 0))


def _tail_events(seed, draws):
    """Draws of the stream's first `draws` that are a tail event of the draw pass: layer 0 and rabs >= ki[0] (every such draw is
    evaluated, whether or not an attempt starts there: tools/np_draw_fixed_work.py counts them the same way)."""
    raw = np.random.default_rng(seed).bit_generator.random_raw(int(draws))
    layer0 = (raw & np.uint64(0xff)) == 0
    rabs = (raw[layer0] >> np.uint64(9)) & np.uint64((1 << 52) - 1)
    return int((rabs >= _ki0()).sum())


def _draw(ctx, seed, std, kind_bits, dst):
    job = N.np_job(N.NP_NORMAL_I16 | kind_bits, N.np_stream(np.random.default_rng(seed)), SAMPLES, std, dst=dst.ptr)
    res = N.VkxNpResult()
    N.check(N.lib().vkx_np_draw_batch_dev(ctx.handle, ctypes.byref(job), 1, ctypes.byref(res)))
    ctx.sync()
    dst.invalidate_host()      # (a DevArray keeps its first download)
    return dst.host(), res


def test_streams_with_1e5_tail_events_match_numpy_on_both_paths():
    ctx = N.default_ctx()
    dst = ctx.dev_empty((SAMPLES,), np.int16)
    tails = 0
    for seed, std in STREAMS:
        ref = np.random.default_rng(seed)
        want = np.round(ref.normal(0, std, SAMPLES)).astype(np.int16)
        state = int(ref.bit_generator.state['state']['state'])
        got, res = _draw(ctx, seed, std, 0, dst)
        bad = int((got != want).sum())
        print(f'seed {seed} std {std}: fast path flags {res.flags} draws {res.draws} mismatches {bad}')
        assert res.flags == 0, (seed, std, res.flags)
        assert bad == 0, (seed, std, bad)
        assert N.pcg64_jump(*N.np_stream(np.random.default_rng(seed)), res.draws) == state, (seed, std)
        draws = int(res.draws)
        # every tail pass through float64: the wedge tests all count as ambiguous under the wide margin, the values are numpy's all the same
        got, res = _draw(ctx, seed, std, WIDE_MARGIN, dst)
        bad = int((got != want).sum())
        print(f'seed {seed} std {std}: float64 path flags {res.flags} draws {res.draws} mismatches {bad}')
        assert res.flags & AMBIGUOUS and not res.flags & SHORT, (seed, std, res.flags)
        assert bad == 0, (seed, std, bad)
        assert int(res.draws) == draws, (seed, std)
        del got, want
        tails += _tail_events(seed, draws)
    print(f'tail events of the {len(STREAMS)} streams ({len(STREAMS) * SAMPLES} samples): {tails}')
    assert tails >= 100_000, tails


def test_log_estimate_error_is_a_quarter_of_the_bound():
    """tail_log_est against -log1p(-u) in float64 on 1.2e7 arguments: uniform u, u within 2^-30 of 0 and of 1, the ends included."""
    ctx = N.default_ctx()
    rng = np.random.default_rng(2024)
    n = 4_000_000
    uniform = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    near0 = rng.integers(0, 1 << 23, n, dtype=np.uint64) << np.uint64(11)
    near1 = (np.uint64((1 << 53) - 1) - rng.integers(0, 1 << 23, n, dtype=np.uint64)) << np.uint64(11)
    near0[:2] = [0, 1 << 11]
    near1[:2] = [(1 << 64) - 1, ((1 << 53) - 1) << 11]
    worst = 0.0
    eps = ctypes.c_double(0.0)
    for name, draws in (('uniform', uniform), ('u < 2^-30', near0), ('1 - u <= 2^-30', near1)):
        u = (draws >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
        assert name == 'uniform' or (u < 2.0 ** -30).all() or (1.0 - u <= 2.0 ** -30).all()
        src = ctx.to_device(draws)
        est = ctx.dev_empty((n,), np.float64)
        N.check(N.lib().vkx_np_tail_log_est_dev(ctx.handle, ctypes.c_void_p(src.ptr), n, ctypes.c_void_p(est.ptr), ctypes.byref(eps)))
        ctx.sync()
        err = float(np.abs(est.host() - (-np.log1p(-u))).max())
        print(f'{name}: largest |estimate - (-log1p(-u))| = {err:.4g} = {err / eps.value:.4f} eps (eps = {eps.value:.6g})')
        worst = max(worst, err)
    print(f'largest error of the estimate on {3 * n} arguments: {worst:.4g} = {worst / eps.value:.4f} eps')
    assert 0.0 < eps.value <= 2.0 ** -12
    assert worst <= eps.value / 4, (worst, eps.value)
