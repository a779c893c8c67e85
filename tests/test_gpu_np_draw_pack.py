"""The int16 draw pass (k_np_draw_compact) parks two rounds of a lane per LDS dword and squeezes a tile's samples together from
that layout.  Streams whose lengths end inside a tile, inside a round, on an odd and on an even round -- 64 draws per round,
48 rounds per tile -- against numpy itself: every value and the generator state after the call."""
import ctypes

import numpy as np
import pytest

from vkit_amd import _native as N

pytestmark = pytest.mark.gpu

ROUND, TILE = 64, 64 * 48
LENGTHS = [
    1, 63, 65, 127, 129,                  # inside the first pair of rounds
    TILE - 1, TILE, TILE + 1,             # around a tile boundary
    5 * TILE + 17 * ROUND + 33,           # mid tile, mid round of an odd round
    3 * TILE + 24 * ROUND,                # on the boundary of an even round
    2 * TILE + 47 * ROUND + 63,           # the last (odd) round of a tile
    9 * TILE + 46 * ROUND + 5,            # the last even round of a tile
    1_000_003,
]


def _same_state(a, b):
    return a.bit_generator.state == b.bit_generator.state


@pytest.mark.parametrize('std', [1.0, 10.0, 14.0])
@pytest.mark.parametrize('seed', [3, 1234, 987_654_321])
def test_int16_plane_lengths_match_numpy(seed, std):
    for n in LENGTHS:
        rng, ref = np.random.default_rng(seed + n), np.random.default_rng(seed + n)
        want = np.round(ref.normal(0, std, n)).astype(np.int16)
        got = N.np_normal_i16((n,), std, rng)
        assert got is not None, n
        assert (got == want).all(), n
        assert _same_state(rng, ref), n


@pytest.mark.parametrize('std', [1.0, 10.0, 14.0])
def test_tile_slots_match_numpy(std):
    """VKX_NP_NORMAL_TILES: the compacted slots themselves, read back through the documented layout."""
    ctx = N.default_ctx()
    for i, n in enumerate(LENGTHS):
        rng, ref = np.random.default_rng(50 + i), np.random.default_rng(50 + i)
        want = np.round(ref.normal(0, std, n)).astype(np.int16)
        buf = np.zeros(N.np_tiles_layout(n)[4], np.uint8)
        job = N.np_job(N.NP_NORMAL_TILES, N.np_stream(rng), n, std, dst=N._ptr(buf))
        res = N.VkxNpResult()
        N.check(N.lib().vkx_np_draw(ctx.handle, ctypes.byref(job), ctypes.byref(res)))
        assert res.flags == 0 and res.samples >= n, n
        assert (N.np_tiles_plane(buf, n) == want).all(), n
        N.np_consume(rng, res.draws)
        assert _same_state(rng, ref), n


def test_noise_added_to_pixels_matches_numpy():
    """The in-place add onto uint8 pixels (gaussion_noise) of planes whose sizes end mid tile."""
    for seed, (h, w), std in ((1, (97, 61), 1.0), (2, (301, 211), 10.0), (3, (517, 389), 14.0)):
        img = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
        rng, ref = np.random.default_rng(seed), np.random.default_rng(seed)
        got = N.np_gaussion_noise(img, std, rng)
        want = np.clip(img.astype(np.int16) + np.round(ref.normal(0, std, img.shape)).astype(np.int16), 0, 255).astype(np.uint8)
        assert (got == want).all() and _same_state(rng, ref)


def test_wide_margin_still_hands_back_to_numpy():
    """VKX_NP_DEBUG_WIDE_MARGIN: every wedge test is declared ambiguous, the call is refused and the generator left alone, and the
    values the device wrote are numpy's all the same."""
    ctx = N.default_ctx()
    for seed, n, std in ((9, 5 * TILE + 17 * ROUND + 33, 14.0), (10, 2 * TILE + 47 * ROUND + 63, 1.0)):
        rng = np.random.default_rng(seed)
        before = rng.bit_generator.state
        dst = ctx.pinned_empty((n,), np.int16)
        job = N.np_job(N.NP_NORMAL_I16 | 0x100, N.np_stream(rng), n, std, dst=N._ptr(dst))
        res = N.VkxNpResult()
        N.check(N.lib().vkx_np_draw(ctx.handle, ctypes.byref(job), ctypes.byref(res)))
        assert res.flags & N.NP_AMBIGUOUS
        assert rng.bit_generator.state == before
        assert (dst == np.round(np.random.default_rng(seed).normal(0, std, n)).astype(np.int16)).all()
