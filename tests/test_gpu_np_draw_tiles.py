"""The int16 draw pass (k_np_draw_compact) at its tile boundaries, against numpy itself.

A wavefront of the draw pass walks a run of consecutive tiles and carries the generator state of its lanes from one tile into the
next; a new job inside a run starts again from the job's tile states.  These tests pin the streams where that matters: lengths
that end on a tile's first sample, one before and one after it; carry-in across the tiles of a run; runs that cross from one job
into the next; a tile with more than 64 attempts that are not a fast accept."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from vkit_amd import _native as N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 3072          # raw draws per tile (64 lanes x VKX_NP_ROUNDS = 48)


def _tiles_buffer(seed, n, std):
    ctx = N.default_ctx()
    rng = np.random.default_rng(seed)
    buf = np.zeros(N.np_tiles_layout(n)[4], np.uint8)
    job = N.np_job(N.NP_NORMAL_TILES, N.np_stream(rng), n, std, dst=N._ptr(buf))
    res = N.VkxNpResult()
    N.check(N.lib().vkx_np_draw(ctx.handle, ctypes.byref(job), ctypes.byref(res)))
    return buf, res


def _first_samples(seed, n, std):
    """Index of every tile's first sample (the buffer's table), from one draw of n samples."""
    buf, res = _tiles_buffer(seed, n, std)
    tiles, _, table_off, _, _ = N.np_tiles_layout(n)
    return buf[table_off:table_off + 8 * (tiles + 1)].view(np.uint32).reshape(tiles + 1, 2)[:, 0].astype(np.int64)


def _ki():
    text = open(os.path.join(ROOT, 'vkit_amd', 'csrc', 'np_ziggurat.h')).read()
    body = re.search(r'kNpZigK\[256\]\s*=\s*\{(.*?)\}', text, re.S).group(1)
    return np.array([int(v.strip().rstrip('uUlL'), 0) for v in body.split(',') if v.strip()], np.uint64)


def _slow_per_tile(seed, tiles):
    """Draws per tile whose attempt is not a fast accept (the draw pass's events), from numpy's raw stream."""
    raw = np.random.default_rng(seed).bit_generator.random_raw(tiles * TILE).astype(np.uint64)
    idx = (raw & np.uint64(0xff)).astype(np.int64)
    rabs = (raw >> np.uint64(9)) & np.uint64((1 << 52) - 1)
    return (rabs >= _ki()[idx]).reshape(tiles, TILE).sum(axis=1)


def _around_a_tile_boundary(std):
    # (the streams of k = 1 and 2 span at most 8 tiles: one tile per wavefront whatever VKX_NP_TPW says; k = 17 and 33 are the
    # lengths whose wavefronts walk runs of several tiles under VKX_NP_TPW=4)
    seed = 41
    first = _first_samples(seed, 40 * TILE, std)
    for k in (1, 2, 17, 33):
        for n in (int(first[k]) - 1, int(first[k]), int(first[k]) + 1):
            rng, ref = np.random.default_rng(seed), np.random.default_rng(seed)
            want = np.round(ref.normal(0, std, n)).astype(np.int16)
            got = N.np_normal_i16((n,), std, rng)
            assert got is not None and (got == want).all(), (k, n)
            assert rng.bit_generator.state == ref.bit_generator.state, (k, n)


@pytest.mark.parametrize('std', [3.0, 10.0])
def test_lengths_around_a_tile_boundary(std):
    _around_a_tile_boundary(std)


@pytest.mark.parametrize('std', [3.0, 10.0])
def test_lengths_around_a_tile_boundary_in_runs(std):
    """The same with four tiles per wavefront (VKX_NP_TPW is read once per process: a child process), so that the tiles after
    the first of a run start from the state the walk of their predecessor left."""
    code = f'import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, "tests")!r}]; import test_gpu_np_draw_tiles as T; T._around_a_tile_boundary({std})'
    out = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, VKX_NP_TPW='4'), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr


def test_tile_with_more_than_64_events():
    seed = next(s for s in range(1000, 2000) if _slow_per_tile(s, 64).max() > 64)
    slow = _slow_per_tile(seed, 64)
    n = 64 * TILE
    rng, ref = np.random.default_rng(seed), np.random.default_rng(seed)
    want = np.round(ref.normal(0, 10.0, n)).astype(np.int16)
    got = N.np_normal_i16((n,), 10.0, rng)
    assert got is not None and (got == want).all(), int(np.argmax(slow))
    assert rng.bit_generator.state == ref.bit_generator.state


_RUNS = r'''
import ctypes, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from vkit_amd import _native as N
ctx = N.default_ctx()
sizes = [1, 2, 3005, 3006, 3072, 6013, 9100, 40_000, 123_457] + [20_000 + 1_777 * k for k in range(40)]
B = len(sizes)
jobs = (N.VkxNpJob * B)()
res = N.NpResults(ctx, B)
outs = []
for i, n in enumerate(sizes):
    d = ctx.dev_empty((N.np_tiles_layout(n)[4],), np.uint8)
    outs.append(d)
    jobs[i] = N.np_job(N.NP_NORMAL_TILES, N.np_stream(np.random.default_rng(900 + i)), n, 2.0 + i % 9, dst=d.ptr)
N.check(N.lib().vkx_np_draw_batch_dev(ctx.handle, jobs, B, res.array))
ctx.sync()
for i, n in enumerate(sizes):
    assert res[i].flags == 0, i
    want = np.round(np.random.default_rng(900 + i).normal(0, 2.0 + i % 9, n)).astype(np.int16)
    assert (N.np_tiles_plane(outs[i].host(), n) == want).all(), (i, n)
print('ok', B)
'''


@pytest.mark.parametrize('tpw', ['2', '4'])
def test_runs_of_tiles_across_jobs(tpw):
    """A batch of ragged streams with two and four tiles per wavefront (VKX_NP_TPW, read once per process: a child process): runs
    start inside a job, cross into the next one and end inside it."""
    env = dict(os.environ, VKX_NP_TPW=tpw)
    out = subprocess.run([sys.executable, '-c', _RUNS, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith('ok')


def test_walks_with_a_carry_in():
    """The start resolution of phase 3 is shared with the walks that take a carry-in (c_in > 0: the previous tile's last attempt
    consumed the tile's first draws): k_np_resolve re-simulates such tiles (kCount) and k_np_place_walk emits the speckle plane
    from them (kEmit).  A speckle plane of 3 M samples whose stream has attempts that end past a tile's last draw, against numpy."""
    img = np.random.default_rng(5).integers(1, 256, (1024, 1024, 3), dtype=np.uint8)
    tiles = img.size // TILE
    seed = next(s for s in range(60, 200) if (_last_draw_slow(s, tiles)).sum() >= 3)
    rng, ref = np.random.default_rng(seed), np.random.default_rng(seed)
    got = N.np_speckle_noise(img, 0.3, rng)
    assert got is not None
    m = img.astype(np.float32)
    want = np.clip(m + m * ref.normal(0, 0.3, m.shape), 0, 255).astype(np.uint8)
    assert (got == want).all()
    assert rng.bit_generator.state == ref.bit_generator.state


def _last_draw_slow(seed, tiles):
    """Per tile: its last draw is not a fast accept (an attempt there, if it starts, consumes the next tile's first draw)."""
    raw = np.random.default_rng(seed).bit_generator.random_raw(tiles * TILE).astype(np.uint64).reshape(tiles, TILE)[:, -1]
    idx = (raw & np.uint64(0xff)).astype(np.int64)
    rabs = (raw >> np.uint64(9)) & np.uint64((1 << 52) - 1)
    return rabs >= _ki()[idx]
