"""The head of phase E of the chain's pixel kernels (csrc/fused.hip): a workgroup reads the descriptor fields of its own item in one
scalar fetch, and a wavefront asks for the noise of its eight output rows back to back -- row i = (row in tile) // 8 from a scalar
row base plus the lane's offset, with a step for the lanes beyond a generator tile boundary -- and waits row by row.  Every result
here equals the oracle chain remap -> gaussian_blur -> color_shift_rgb -> add_noise_i16 (-> line_streak) byte for byte: rows that
cross a generator tile in every one of the eight row slots, in interior and in border tiles, and batches whose neighbouring items
differ in every field of that fetch.  Both cases run through the single kernel (k_chain_fused_whole) and through the split ones
(k_chain_fused, _rim, _over)."""
import numpy as np
import pytest
from numpy.random import default_rng

import oracle as O

pytestmark = pytest.mark.gpu

TILE = 60            # tile side of the 5-tap chain: the 64-pixel window minus the blur halo (csrc/fused.hip tile_side)
R = 2
STD = 11.0
KSIZES = (1, 3, 5, 7)
# the small level-5 camera states of test_gpu_chain_noise_groups.py: sides between 97 and 200 px.  The numpy streams 7000 + k give these
# results a generator tile boundary every 5 to 10 rows.  Walked on the CPU with the oracle's stream restatement (np_normal_i16, 3072
# raw draws per generator tile) before the seeds were fixed, the boundaries inside whole 4-pixel groups fall into every row slot 8 to
# 27 times in border tiles and 1 to 4 times in interior tiles, and three times on row 0 of a tile.  The test counts them again in
# the device's table.
SHAPES = [(97, 200), (130, 163), (200, 98), (151, 121), (112, 187), (185, 140), (99, 177), (166, 118)]
LINE = dict(thickness=2, gap=9, dash_thickness=3, dash_gap=5, alpha=0.6, color=(10, 200, 30), enable_vert=True, enable_hori=True)


def _reached(dv, dshape):
    """Which tiles of a result hold a lattice cell, as k_chain_setup bins them: a cell belongs to every tile whose window meets the
    bounding box of its four destination vertices."""
    dh, dw = dshape
    tiles_y, tiles_x = -(-dh // TILE), -(-dw // TILE)
    reached = np.zeros((tiles_y, tiles_x), bool)
    quads = np.stack([dv[:-1, :-1], dv[:-1, 1:], dv[1:, 1:], dv[1:, :-1]], 2).reshape(-1, 4, 2)
    for q in quads:
        xmin, xmax, ymin, ymax = int(q[:, 0].min()), int(q[:, 0].max()), int(q[:, 1].min()), int(q[:, 1].max())
        tx0, ty0 = max(xmin - R, 0) // TILE, max(ymin - R, 0) // TILE
        tx1, ty1 = min((xmax + R) // TILE, tiles_x - 1), min((ymax + R) // TILE, tiles_y - 1)
        if tx0 <= tx1 and ty0 <= ty1:
            reached[ty0:ty1 + 1, tx0:tx1 + 1] = True
    return reached


@pytest.fixture(scope='module')
def cases():
    """Eight level-5 camera_cubic_curve states, their noise planes and the oracle's remap blurred with every kernel size."""
    from vkit_amd.mechanism import distortion as D
    from vkit_amd.mechanism.distortion_policy.geometric import camera as P_cam
    rng = default_rng(2024)
    out = []
    for k, shape in enumerate(SHAPES):
        cfg = P_cam.CameraCubicCurveConfigGenerator(P_cam.CameraCubicCurveConfigGeneratorConfig(), 5)(shape, rng)
        st = D.camera_cubic_curve.generate_state(cfg, shape)
        image = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
        mx, my = O.grid_to_map(st.src_image_grid.vertices, st.dst_image_grid.vertices, st.result_shape)
        remapped = O.remap(image, mx, my)
        blurred = {ks: O.gaussian_blur(remapped, ks, 1.0) if ks > 1 else remapped for ks in KSIZES}
        plane = np.round(default_rng(7000 + k).normal(0, STD, tuple(st.result_shape) + (3,))).astype(np.int16)
        out.append(dict(image=image, state=st, seed=7000 + k, plane=plane, blurred=blurred))
    return out


@pytest.fixture(params=['0', '1'], ids=['whole', 'split'])
def split(request, monkeypatch):
    """VKX_CHAIN_SPLIT (read at every call): 0 = k_chain_fused_whole, 1 = k_chain_fused + _rim + _over."""
    monkeypatch.setenv('VKX_CHAIN_SPLIT', request.param)
    return request.param


def test_crossings_in_every_row_slot(cases, split):
    from vkit_amd import _native as N
    from vkit_amd.batch import ChainBatch
    batch = ChainBatch()
    for c in cases:
        batch.add(c['image'], c['state'], blur_sigma=1.0, hue_delta=37, noise_std=STD, noise_rng=default_rng(c['seed']))
    batch.run()
    got = [batch.result(k) for k in range(len(cases))]
    assert batch.stream_fallbacks == 0 and all(it.noise_tiled == 1 and it.blur_ksize == 5 for it in batch._items)
    slots = {'interior': set(), 'border': set()}       # wavefront row slots (row in tile) // 8 of the crossing rows, by tile class
    first_rows = 0                                       # crossings on output row 0 of a tile
    for k, c in enumerate(cases):
        dh, dw = c['state'].result_shape
        n = dh * dw * 3
        tiles, _slot, table_off, _slots_off, nbytes = N.np_tiles_layout(n)
        buf = batch.ctx.download(batch._items[k].noise, np.empty(nbytes, np.uint8))
        assert (N.np_tiles_plane(buf, n) == c['plane'].reshape(-1)).all(), k
        table = buf[table_off:table_off + 8 * (tiles + 1)].view(np.uint32).reshape(tiles + 1, 2)
        reached = _reached(np.asarray(c['state'].dst_image_grid.vertices), (dh, dw))
        for t in range(1, tiles):
            b = int(table[t, 0])              # first sample of generator tile t
            if b >= n:
                break
            y, s = divmod(b, dw * 3)
            tx = s // (3 * TILE)
            r = s - tx * 3 * TILE             # the boundary's sample index within the row segment of its tile column
            full4 = min(TILE, dw - tx * TILE) & ~3
            ty, ry = divmod(y, TILE)
            if not (0 < r < 3 * full4 and reached[ty, tx]):
                continue                      # (not inside whole 4-pixel groups, or an empty tile)
            wx0, wy0 = tx * TILE - R, ty * TILE - R
            inside = wx0 >= 0 and wy0 >= 0 and wx0 + 64 <= dw and wy0 + 64 <= dh
            slots['interior' if inside else 'border'].add(ry // 8)
            first_rows += ry == 0
        want = O.add_noise_i16(O.color_shift_rgb(c['blurred'][5], 37), c['plane'])
        assert got[k].shape == want.shape and (got[k] == want).all(), k
    batch.close()
    assert slots['interior'] | slots['border'] == set(range(8)), slots
    assert slots['border'] == set(range(8)) and len(slots['interior']) >= 4, slots
    assert first_rows > 0


def _odd_pitch_plane(batch, idx, plane):
    """The item's noise as an int16 plane with an odd pitch whose last row ends on the last element of its allocation; the padding
    between the rows holds a value that would show in the result."""
    dh, dw = plane.shape[:2]
    stride = dw * 3 + 3
    stride += 1 - stride % 2
    padded = np.full((dh, stride), 12345, np.int16)
    padded[:, :dw * 3] = plane.reshape(dh, dw * 3)
    flat = padded.reshape(-1)[:(dh - 1) * stride + dw * 3]
    ptr = batch.ctx.malloc(flat.nbytes)
    batch._owned.append(ptr)
    batch.ctx.upload(ptr, flat)
    batch._items[idx].noise, batch._items[idx].noise_stride_el = ptr, stride
    assert stride % 2 == 1


@pytest.mark.parametrize('streak', [False, True], ids=['plain', 'streak'])
def test_mixed_descriptors_in_one_batch(cases, split, streak):
    """Neighbouring items differ in the hue member (on / off), the noise form (tile slots, int16 plane with an odd pitch, none) and
    the blur radius (0 - 3): a workgroup that fetched another item's fields would show in its tile."""
    from vkit_amd.batch import ChainBatch
    from vkit_amd.mechanism.distortion.photometric.streak import LineStreakConfig
    batch = ChainBatch()
    wants = []
    forms = set()
    for k, c in enumerate(cases):
        hue = 37 + k if k % 2 == 0 else None
        form = ('tiled', 'plane', 'none')[k % 3]
        ksize = KSIZES[(k + 2) % 4]
        line = LineStreakConfig(**LINE) if streak and k % 4 < 2 else None
        noise = dict(noise_std=STD, noise_rng=default_rng(c['seed'])) if form == 'tiled' else dict(noise=c['plane']) if form == 'plane' else {}
        idx = batch.add(c['image'], c['state'], blur_sigma=1.0, hue_delta=hue, streak=line, **noise)
        batch._items[idx].blur_ksize = ksize if ksize > 1 else 0      # (ChainBatch.add derives the size from sigma)
        batch._items[idx].blur_sigma = 1.0 if ksize > 1 else 0.0
        batch._array = None
        if form == 'plane':
            _odd_pitch_plane(batch, idx, c['plane'])
        want = c['blurred'][ksize]
        if hue is not None:
            want = O.color_shift_rgb(want, hue)
        if form != 'none':
            want = O.add_noise_i16(want, c['plane'])
        if line is not None:
            want = O.line_streak(want, 2, 9, 3, 5, (10, 200, 30), 0.6, True, True)
        wants.append(want)
        forms.add((hue is not None, form, ksize // 2))
    assert {f[1] for f in forms} == {'tiled', 'plane', 'none'} and {f[2] for f in forms} == {0, 1, 2, 3} and {f[0] for f in forms} == {False, True}
    batch.run()
    assert batch.stream_fallbacks == 0
    assert [it.noise_tiled for it in batch._items] == [int(k % 3 == 0) for k in range(len(cases))]
    for k, want in enumerate(wants):
        got = batch.result(k)
        assert got.shape == want.shape and (got == want).all(), (k, split, streak)
    batch.close()
