"""Phase 1 of the numpy-stream draw pass (csrc/nprand.hip, walk_tile): the draw rotated once by r + 9, the fast accept's value as one
fma against a table of -2^52 wi with the sign put on the product, and the stride step's two carry chains.  Every value and the generator
position against numpy ITSELF -- np.round(default_rng(seed).normal(0, std, n)).astype(int16) --, in the plain int16 form, in the
tile-slot form, and through the chain that reads the slots; lengths of one lane, around the tile edges (3072 raw draws per tile) and of
more than 13 tiles; generator states set by hand whose limbs are all zeros, all ones or alternate, with several odd increments."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
from numpy.random import default_rng

import oracle as O
from vkit_amd import _native as N

pytestmark = pytest.mark.gpu

LENGTHS = (1, 63, 64, 65, 3071, 3072, 3073, 6145, 40_000)
STDS = (0.5, 1.0, 10.0, 37.5, 300.0)
M128 = (1 << 128) - 1
STATES = (0, M128, (1 << 64) - 1, 0xffffffff00000000ffffffff00000000, 0x00000000ffffffff00000000ffffffff)
INCS = (1, M128, 0xffffffff00000000ffffffff00000001, 0x5851f42d4c957f2d14057b7ef767814f)


def _plain(rng, n, std):
    got = N.np_normal_i16((n,), std, rng)
    assert got is not None
    return got


def _tiles(rng, n, std):
    """The plane a VKX_NP_NORMAL_TILES job leaves in its slots, read through the documented layout; moves `rng` as numpy would."""
    ctx = N.default_ctx()
    nbytes = N.np_tiles_layout(n)[4]
    buf = np.zeros(nbytes, np.uint8)
    job = N.np_job(N.NP_NORMAL_TILES, N.np_stream(rng), n, std, dst=N._ptr(buf))
    res = N.VkxNpResult()
    N.check(N.lib().vkx_np_draw(ctx.handle, ctypes.byref(job), ctypes.byref(res)))
    assert res.flags == 0 and res.samples >= n
    N.np_consume(rng, res.draws)
    return N.np_tiles_plane(buf, n)


def _check(form, make_rng, n, std):
    rng, ref = make_rng(), make_rng()
    want = np.round(ref.normal(0, std, n)).astype(np.int16)
    got = form(rng, n, std)
    assert (got == want).all()
    assert rng.bit_generator.state == ref.bit_generator.state
    return want


@pytest.mark.parametrize('form', [_plain, _tiles], ids=['plain', 'tiles'])
@pytest.mark.parametrize('std', STDS)
@pytest.mark.parametrize('n', LENGTHS)
def test_lengths_and_deviations_match_numpy(n, std, form):
    seed = 100_000 + 1000 * LENGTHS.index(n) + STDS.index(std)
    _check(form, lambda: default_rng(seed), n, std)


def test_long_stream_takes_every_rotation_both_signs_and_the_tail():
    """What the 40 000-draw cases are said to cover, counted on the stream itself (PCG64 XSL-RR restated: the rotation amount is the
    top six bits of the state, idx / sign / rabs the low 61 bits of the rotated word)."""
    st = default_rng(100_000 + 1000 * LENGTHS.index(40_000)).bit_generator.state['state']
    s, inc = int(st['state']), int(st['inc'])
    rot = np.zeros(64, np.int64)
    neg = tail = 0
    for _ in range(40_000):
        s = (s * N._PCG_MULT + inc) & M128
        hi, lo = s >> 64, s & N._M64
        r = hi >> 58
        x = hi ^ lo
        u = ((x >> r) | (x << (64 - r))) & N._M64
        rot[r] += 1
        neg += (u >> 8) & 1
        tail += (u & 0xff) == 0
    assert rot.min() >= 400 and rot[55:].min() >= 400
    assert 19_000 < neg < 21_000
    assert tail >= 3          # layer 0: some of them are tail events


@pytest.mark.parametrize('form', [_plain, _tiles], ids=['plain', 'tiles'])
@pytest.mark.parametrize('inc', INCS, ids=lambda v: f'inc{v & 0xffff:04x}{v >> 112:04x}')
@pytest.mark.parametrize('state', STATES, ids=lambda v: f'state{v & 0xffff:04x}{v >> 112:04x}')
def test_hand_made_states_match_numpy(state, inc, form):
    def make():
        rng = default_rng(0)
        rng.bit_generator.state = {'bit_generator': 'PCG64', 'state': {'state': state, 'inc': inc}, 'has_uint32': 0, 'uinteger': 0}
        return rng
    _check(form, make, 6145, 10.0)


def test_chain_reads_the_slots_of_every_deviation():
    """One image of 130 x 150 px per deviation in one batch: remap -> blur -> hue -> + the stream's noise, read from the generator's tile
    slots by the chain kernel, against the oracle chain with numpy's plane."""
    from vkit_amd.batch import ChainBatch
    rng = default_rng(14)
    H, W = 130, 150
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    ys = list(range(0, H, 16)) + [H - 1]
    xs = list(range(0, W, 16)) + [W - 1]
    sv = np.array([[(x, y) for x in xs] for y in ys], np.int32)
    dv = sv + rng.integers(-5, 6, sv.shape)
    dv[..., 0] -= dv[..., 0].min()
    dv[..., 1] -= dv[..., 1].min()
    dshape = (int(dv[..., 1].max()) + 1, int(dv[..., 0].max()) + 1)
    state = SimpleNamespace(result_shape=dshape, src_image_grid=SimpleNamespace(vertices=sv), dst_image_grid=SimpleNamespace(vertices=dv))
    mx, my = O.grid_to_map(sv, dv, dshape)
    base = O.color_shift_rgb(O.gaussian_blur(O.remap(img, mx, my), 5, 1.0), 37)
    batch = ChainBatch()
    for k, std in enumerate(STDS):
        batch.add(img, state, blur_sigma=1.0, hue_delta=37, noise_std=std, noise_rng=default_rng(200_000 + k))
    batch.run()
    assert batch.stream_fallbacks == 0 and all(it.noise_tiled == 1 for it in batch._items)
    for k, std in enumerate(STDS):
        plane = np.round(default_rng(200_000 + k).normal(0, std, dshape + (3,))).astype(np.int16)
        assert (batch.result(k) == O.add_noise_i16(base, plane)).all(), std
    batch.close()
