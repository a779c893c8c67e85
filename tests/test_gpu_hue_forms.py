"""The hue round trip of csrc/vkx_color.h in its cheaper forms (the interpolation factor from an exponent-trick float without
convert, compare or select, the shift on the rounding term of the hue product), run by every kernel that holds it and compared
with the oracle byte for byte: the single-stage colour shift of photo.hip on the image of all 2^24 RGB triples, and the fused
chain through k_chain_fused + k_chain_fused_rim + k_chain_fused_over (VKX_CHAIN_SPLIT=1) and k_chain_fused_whole (=0), the
streak instances included.  tests/test_hue_forms_exhaustive.py proves the same source lines on the CPU."""
from types import SimpleNamespace

import numpy as np
import pytest
from numpy.random import default_rng

import oracle as O

pytestmark = pytest.mark.gpu

STD = 11.0
LINE = dict(thickness=2, gap=9, dash_thickness=3, dash_gap=5, alpha=0.6, color=(10, 200, 30), enable_vert=True, enable_hori=True)


# ------------------------------------------------------------------------------------------ single stage
@pytest.fixture(scope='module')
def all_triples():
    v = np.arange(256, dtype=np.uint8)
    return np.ascontiguousarray(np.stack(np.meshgrid(v, v, v, indexing='ij'), -1).reshape(4096, 4096, 3))


@pytest.mark.parametrize('delta', [1, 37, 255])
def test_single_stage_colour_shift_on_every_triple(all_triples, delta):
    from vkit_amd import _native as N
    got = N.color_shift_rgb(all_triples, delta)
    want = O.color_shift_rgb(all_triples, delta)
    assert (got == want).all(), (delta, int((got != want).any(-1).sum()))


# ------------------------------------------------------------------------------------------ chain
def _edges(n, step):
    e = [0]
    while e[-1] < n - 1:
        e.append(min(e[-1] + step(e[-1]), n - 1))
    return e


def _lattice(edges_x, edges_y, seed):
    """A hand-built lattice (as in tests/test_gpu_chain_split.py): source vertices on the given edges, destination vertices one
    pixel off them at most."""
    sv = np.array([[(x, y) for x in edges_x] for y in edges_y], np.int32)
    px, py = default_rng(seed).uniform(0, 6.28, 2)
    dv = sv.copy()
    dv[..., 0] += np.rint(1.2 * np.sin(sv[..., 1] / 37.0 + px)).astype(np.int32)
    dv[..., 1] += np.rint(1.2 * np.cos(sv[..., 0] / 29.0 + py)).astype(np.int32)
    dv[..., 0] -= dv[..., 0].min()
    dv[..., 1] -= dv[..., 1].min()
    return sv, dv, (int(dv[..., 1].max()) + 1, int(dv[..., 0].max()) + 1)


def _census(dv, dshape, R):
    """Tile classes as the kernels see them (k_chain_setup's binning rule): a tile's candidate count is the bounding rectangle,
    in lattice rows x columns, of the cells whose destination box, widened by the blur radius, meets it."""
    dh, dw = dshape
    T = (64 - 2 * R) & ~3
    tiles_y, tiles_x = -(-dh // T), -(-dw // T)
    rmin = np.full((tiles_y, tiles_x), 1 << 30); cmin = rmin.copy()
    rmax = np.full((tiles_y, tiles_x), -1); cmax = rmax.copy()
    quads = np.stack([dv[:-1, :-1], dv[:-1, 1:], dv[1:, 1:], dv[1:, :-1]], 2)
    xmin, xmax = quads[..., 0].min(-1), quads[..., 0].max(-1)
    ymin, ymax = quads[..., 1].min(-1), quads[..., 1].max(-1)
    for r in range(quads.shape[0]):
        for c in range(quads.shape[1]):
            tx0, ty0 = max(int(xmin[r, c]) - R, 0) // T, max(int(ymin[r, c]) - R, 0) // T
            tx1, ty1 = min((int(xmax[r, c]) + R) // T, tiles_x - 1), min((int(ymax[r, c]) + R) // T, tiles_y - 1)
            if tx0 <= tx1 and ty0 <= ty1:
                s = (slice(ty0, ty1 + 1), slice(tx0, tx1 + 1))
                rmin[s] = np.minimum(rmin[s], r); rmax[s] = np.maximum(rmax[s], r)
                cmin[s] = np.minimum(cmin[s], c); cmax[s] = np.maximum(cmax[s], c)
    nc = np.where(rmax >= 0, (rmax - rmin + 1) * (cmax - cmin + 1), 0)
    ty, tx = np.mgrid[:tiles_y, :tiles_x]
    rect = (tx * T - R >= 0) & (ty * T - R >= 0) & (tx * T - R + 64 <= dw) & (ty * T - R + 64 <= dh)
    return dict(interior=int((rect & (nc > 0) & (nc <= 64)).sum()), overfull=int((rect & (nc > 64)).sum()),
                rim=int((~rect & (nc > 0)).sum()), ragged=dw % 4 != 0)


# (name, blur kernel size, hue delta, noise from a numpy stream, streak)
CASES = [('r0_hue37', 1, 37, False, False), ('r2_hue200', 5, 200, False, False), ('r2_hue37_noise', 5, 37, True, False),
         ('r2_hue37_noise_streak', 5, 37, True, True)]


@pytest.fixture(scope='module')
def chain_inputs():
    """Two random images: 61 x 67 on a lattice of 16-px cells (rim tiles only, ragged tail columns), 200 x 130 on a lattice of
    cells 10 px wide, 5 px high in the upper rows and 16 px below: its interior rectangle holds tiles with at most 64 candidate
    cells and overfull ones, with and without the blur.  The references of every case, computed once."""
    images = []
    for k, (h, w, step_x, step_y) in enumerate([(61, 67, lambda x: 16, lambda y: 16),
                                                (200, 130, lambda x: 10, lambda y: 5 if y < 110 else 16)]):
        sv, dv, dshape = _lattice(_edges(w, step_x), _edges(h, step_y), 90 + k)
        image = default_rng(70 + k).integers(0, 256, (h, w, 3), dtype=np.uint8)
        mx, my = O.grid_to_map(sv, dv, dshape)
        plain = O.remap(image, mx, my)
        blurred = O.gaussian_blur(plain, 5, 1.0)
        plane = np.round(default_rng(8400 + k).normal(0, STD, dshape + (3,))).astype(np.int16)
        wants = {}
        for name, ksize, hue, noise, streak in CASES:
            want = O.color_shift_rgb(blurred if ksize > 1 else plain, hue)
            if noise:
                want = O.add_noise_i16(want, plane)
            if streak:
                want = O.line_streak(want, 2, 9, 3, 5, (10, 200, 30), 0.6, True, True)
            wants[name] = want
        state = SimpleNamespace(result_shape=dshape, src_image_grid=SimpleNamespace(vertices=sv),
                                dst_image_grid=SimpleNamespace(vertices=dv))
        images.append(dict(image=image, state=state, dv=dv, dshape=dshape, seed=8400 + k, wants=wants))
    return images


def test_inputs_hold_every_tile_class(chain_inputs):
    small, large = chain_inputs
    for R in (0, 2):
        a, b = _census(small['dv'], small['dshape'], R), _census(large['dv'], large['dshape'], R)
        assert a['interior'] == 0 and a['overfull'] == 0 and a['rim'] > 0, (R, a)      # no rectangle: the rim kernel alone
        assert b['interior'] > 0 and b['overfull'] > 0 and b['rim'] > 0, (R, b)
    assert small['dshape'][1] % 4 != 0 or large['dshape'][1] % 4 != 0          # tail columns that take the per-pixel form


@pytest.mark.parametrize('split', ['1', '0'])
@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_chain_equals_the_oracle(chain_inputs, monkeypatch, case, split):
    from vkit_amd.batch import ChainBatch
    from vkit_amd.mechanism.distortion.photometric.streak import LineStreakConfig
    name, ksize, hue, noise, streak = case
    monkeypatch.setenv('VKX_CHAIN_SPLIT', split)
    batch = ChainBatch()
    for c in chain_inputs:
        idx = batch.add(c['image'], c['state'], blur_sigma=1.0 if ksize > 1 else None, hue_delta=hue,
                        noise_std=STD if noise else None, noise_rng=default_rng(c['seed']) if noise else None,
                        streak=LineStreakConfig(**LINE) if streak else None)
        batch._items[idx].blur_ksize = ksize if ksize > 1 else 0          # (ChainBatch.add derives the size from sigma)
        batch._items[idx].blur_sigma = 1.0 if ksize > 1 else 0.0
        batch._array = None
    batch.run()
    assert batch.stream_fallbacks == 0
    for k, c in enumerate(chain_inputs):
        got, want = batch.result(k), c['wants'][name]
        assert got.shape == want.shape and (got == want).all(), (name, split, k, int((got != want).any(-1).sum()))
    batch.close()
