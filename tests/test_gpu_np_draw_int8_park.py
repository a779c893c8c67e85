"""The draw pass that parks a tile's samples as bytes (csrc/nprand.hip, EmitI16B8): chosen per launch where every job satisfies
3.6541528853610088 |scale| + |loc| <= 127, the int16-parked pass for every other launch.  Every value, the draw count and the generator
position against numpy ITSELF -- np.round(default_rng(seed).normal(0, std, n)).astype(int16) -- through the tile-slot entry that
ChainBatch(noise_rng=...) uses: streams that end inside a tile, at its end and on a 16-byte group edge; a stream at std 34.7 whose plane holds
tail samples beyond a byte (their tiles are marked and walked again); deviations just past the bound; one launch that mixes both kinds of job;
and one ChainBatch that reads the slots.

The jobs of the C entry carry a deviation only (`scale`; the device forms have loc = 0), so a location other than 0 reaches the selection
rule alone: tests/test_np_draw_byte_bound.py calls it with loc = +-20 and more."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
from numpy.random import default_rng

import oracle as O
from vkit_amd import _native as N

pytestmark = pytest.mark.gpu


def _tiles_batch(cases):
    """One vkx_np_draw_batch_dev launch of VKX_NP_NORMAL_TILES jobs, cases = [(seed, n, std)]: planes read through the documented layout."""
    ctx = N.default_ctx()
    B = len(cases)
    jobs = (N.VkxNpJob * B)()
    res = N.NpResults(ctx, B)
    bufs = []
    for i, (seed, n, std) in enumerate(cases):
        d = ctx.dev_empty((N.np_tiles_layout(n)[4],), np.uint8)
        bufs.append(d)
        jobs[i] = N.np_job(N.NP_NORMAL_TILES, N.np_stream(default_rng(seed)), n, std, dst=d.ptr)
    N.check(N.lib().vkx_np_draw_batch_dev(ctx.handle, jobs, B, res.array))
    ctx.sync()
    out = []
    for i, (seed, n, std) in enumerate(cases):
        assert res[i].flags == 0 and res[i].samples >= n
        moved = default_rng(seed)
        N.np_consume(moved, res[i].draws)
        out.append((N.np_tiles_plane(bufs[i].host(), n), moved))
    res.close()
    return out


def _check(cases, planes=None):
    got = _tiles_batch(cases)
    for i, (seed, n, std) in enumerate(cases):
        ref = default_rng(seed)
        want = planes[i] if planes else np.round(ref.normal(0, std, n)).astype(np.int16)
        if planes:
            ref.normal(0, std, n)
        plane, moved = got[i]
        assert (plane == want).all(), (seed, n, std)
        assert moved.bit_generator.state == ref.bit_generator.state, (seed, n, std)      # the returned draw count is numpy's


@pytest.mark.parametrize('n', [1, 7, 3005, 3006, 3007, 3 * 3072 + 5])
def test_std_10_streams_end_inside_a_tile_at_its_end_and_on_a_group_edge(n):
    assert N.lib().vkx_np_parks_as_bytes(10.0, 0.0) == 1
    _check([(310_000 + n, n, 10.0)])


def test_tail_samples_beyond_a_byte_mark_their_tile():
    seed, n, std = 320_007, 200_000, 34.7
    assert N.lib().vkx_np_parks_as_bytes(std, 0.0) == 1
    want = np.round(default_rng(seed).normal(0, std, n)).astype(np.int16)
    assert (np.abs(want.astype(np.int32)) > 127).any()         # numpy's own plane leaves the byte somewhere
    _check([(seed, n, std)], planes=[want])


@pytest.mark.parametrize('std', [34.76, 60.0])
def test_deviations_past_the_bound_keep_the_int16_pass(std):
    assert N.lib().vkx_np_parks_as_bytes(std, 0.0) == 0
    _check([(330_000 + int(std), 10_000, std)])


def test_one_launch_of_a_qualifying_and_another_job():
    assert N.lib().vkx_np_parks_as_bytes(10.0, 0.0) == 1 and N.lib().vkx_np_parks_as_bytes(60.0, 0.0) == 0
    _check([(340_001, 10_000, 10.0), (340_002, 10_000, 60.0), (340_003, 3007, 34.7)])


def test_chain_batch_reads_the_slots():
    """Two images of 200 x 150 px, std 10, in one ChainBatch with noise_rng: remap -> blur -> hue -> + the stream's noise against the oracle
    chain with numpy's plane (the path the chain bench drives)."""
    from vkit_amd.batch import ChainBatch
    rng = default_rng(350_000)
    H, W = 200, 150
    ys = list(range(0, H, 16)) + [H - 1]
    xs = list(range(0, W, 16)) + [W - 1]
    sv = np.array([[(x, y) for x in xs] for y in ys], np.int32)
    dv = sv + rng.integers(-5, 6, sv.shape)
    dv[..., 0] -= dv[..., 0].min()
    dv[..., 1] -= dv[..., 1].min()
    dshape = (int(dv[..., 1].max()) + 1, int(dv[..., 0].max()) + 1)
    state = SimpleNamespace(result_shape=dshape, src_image_grid=SimpleNamespace(vertices=sv), dst_image_grid=SimpleNamespace(vertices=dv))
    mx, my = O.grid_to_map(sv, dv, dshape)
    imgs = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(2)]
    batch = ChainBatch()
    for k, img in enumerate(imgs):
        batch.add(img, state, blur_sigma=1.0, hue_delta=37, noise_std=10.0, noise_rng=default_rng(350_001 + k))
    batch.run()
    assert batch.stream_fallbacks == 0 and all(it.noise_tiled == 1 for it in batch._items)
    for k, img in enumerate(imgs):
        base = O.color_shift_rgb(O.gaussian_blur(O.remap(img, mx, my), 5, 1.0), 37)
        plane = np.round(default_rng(350_001 + k).normal(0, 10.0, dshape + (3,))).astype(np.int16)
        assert (batch.result(k) == O.add_noise_i16(base, plane)).all(), k
    batch.close()
