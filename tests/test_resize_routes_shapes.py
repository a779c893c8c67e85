"""The geometry lists of tests/resize_routes.py still sit on the two row switches of the CUBIC / LANCZOS4 resize -- checked on the
CPU with the helper's own restatement of the row rule, without reading the library's source.

The constants this is about (vkit_amd/csrc/resize.hip): kSepRows = 40, the most source rows a 16-row destination tile of the
separable form may need before the call goes to the direct kernels, and kSepRowsSmall = 24, up to which the uint8 calls take the
24-row instance of the separable kernel.  A list that pins a switch has shapes whose largest tile needs exactly one and two rows
less, the constant itself, and one and two rows more."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resize_routes as R  # noqa: E402

SMALL, FULL = 24, 40      # kSepRowsSmall, kSepRows


def test_rows_needed_on_known_shapes():
    # by hand: 8 -> 16 rows, CUBIC: yofs = floor((y + 0.5) / 2 - 0.5) = -1, 0, 0, 1, 1, .. 6, 6, 7; taps yofs - 1 .. yofs + 2 clipped to 0 .. 7
    assert R.tap_offsets(8, 16).tolist() == [-1, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7]
    assert R.rows_needed(8, 16, 4) == [8] and R.rows_needed(8, 16, 8) == [8]
    # identity: tile rows 16 .. 31 of 48 reach 15 .. 33 (CUBIC), 13 .. 35 (LANCZOS4); the outer tiles are clipped at 0 and 47
    assert R.rows_needed(48, 48, 4) == [18, 19, 17] and R.rows_needed(48, 48, 8) == [20, 23, 19]
    assert R.rows_needed(1, 40, 8) == [1, 1, 1]


def test_band_centres_need_the_stated_rows_in_an_interior_unclipped_tile():
    for code, centres in R.CENTRES.items():
        assert len(centres) == 4 and sorted(centres.values()) == [SMALL, SMALL + 1, FULL, FULL + 1]
        for sh, rows in centres.items():
            assert sh in R.BANDS[code]
            tiles = R.tile_rows(sh, R.BAND_DH, R.TAPS[code])
            assert len(tiles) == 3
            assert max(n for n, _ in tiles) == rows, (code, sh, tiles)
            assert tiles[1] == (rows, True), (code, sh, tiles)          # the middle tile: interior, no tap clipped
    assert R.CENTRES[R.CUBIC] == {52: 24, 54: 25, 96: 40, 98: 41}
    assert R.CENTRES[R.LANCZOS4] == {42: 24, 44: 25, 85: 40, 86: 41}


def test_bands_reach_two_rows_to_either_side_of_both_switches():
    for code, band in R.BANDS.items():
        most = {max(R.rows_needed(sh, R.BAND_DH, R.TAPS[code])) for sh in band}
        for at in (SMALL, FULL):
            assert {at - 1, at, at + 1, at + 2} <= most, (code, at, sorted(most))
        # the same along x in the transposed list, and both lists carry the band
        assert [g[0][0] for g in R.band_geometries(code)] == list(band)
        assert [g[0][1] for g in R.transposed_band_geometries(code)] == list(band)
        for (sh, sw), (dh, dw) in R.band_geometries(code):
            assert (sw, dh, dw) == (70, 40, 67)


def test_the_lists_hold_what_they_are_named_for():
    taps = {(g, c) for g, codes in R.sweep_geometries() for c in codes if c in R.TAPS}
    for g in R.NAN_COLUMN:
        assert (g, R.LANCZOS4) in taps
    assert R.NAN_COLUMN == (((146, 4), (64, 196)), ((127, 1), (202, 197)), ((4, 146), (196, 64)))
    # both forms by the default routing in the x-edge list, for either tap count
    for code, ks in R.TAPS.items():
        forms = {max(R.rows_needed(sh, dh, ks)) > FULL for (sh, _), (dh, _) in R.x_edge_geometries()}
        assert forms == {False, True}, code
    assert {dw for _, (_, dw) in R.x_edge_geometries()} == {63, 64, 65, 66, 67, 127, 129}
    assert {dh for _, (dh, _) in R.x_edge_geometries()} == {17, 33}
    clipped = R.clipped_geometries()
    assert {s for (sh, sw), _ in clipped for s in (sh, sw)} == {1, 2, 3, 5, 7}
    assert {d for _, (dh, dw) in clipped for d in (dh, dw)} >= {1, 2, 3}
    assert any(dh > sh and dw > sw for (sh, sw), (dh, dw) in clipped) and any(dh < sh and dw < sw for (sh, sw), (dh, dw) in clipped)
    ratios = sorted(round(40 / dh, 1) for _, (dh, _) in R.scale_geometries())
    assert ratios == [0.3, 0.5, 1.0, 1.9, 2.0, 2.1, 4.0]
    near = R.near_miss_geometries()
    for g in (((64, 50), (32, 50)), ((64, 66), (32, 32)), ((60, 90), (20, 31)), ((60, 90), (20, 45)), ((60, 90), (20, 90)),
              ((64, 160), (4, 10)), ((64, 64), (32, 32))):
        assert g in near
    assert {(sh % 2, sw % 2) for (sh, sw), _ in near[-4:]} == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_either_statement_of_the_coordinate_gives_the_lists_the_same_offsets():
    """(d + 0.5) * s / d and (d + 0.5) * (1 / (d / s)) differ in the last bit for a few size pairs.  Among the heights used here
    that is 4 -> 196 alone, a LANCZOS4 NaN-column geometry, whose point is that rounding (index 24 lands on a whole number)
    and whose four source rows are all reached by clipped taps either way."""
    pairs = {(sh, dh) for ((sh, sw), (dh, dw)), _ in R.sweep_geometries()}
    differ = set()
    for s, d in pairs:
        plain = np.floor(((np.arange(d, dtype=np.float64) + 0.5) * s / d - 0.5).astype(np.float32)).astype(np.int64)
        if (plain != R.tap_offsets(s, d)).any():
            differ.add((s, d))
    assert differ == {(4, 196)}
    assert R.rows_needed(4, 196, 8) == [4] * 13


def test_sources():
    for kind in R.KINDS:
        a, b = R.source(kind, 9, 11, 1), R.source(kind, 9, 11, 1)
        assert a.shape[:2] == (9, 11) and a.dtype in (np.uint8, np.float32)
        assert a.tobytes() == b.tobytes()                                   # seeded
    assert R.source('stripes_x3', 2, 7, 0)[0, :, 0].tolist() == [255, 255, 0, 255, 255, 0, 255]
    assert R.source('stripes_y4', 6, 2, 0)[:, 1, 3].tolist() == [255, 255, 0, 0, 255, 255]
    assert R.source('stripes_x2', 2, 4, 0)[1, :, 2].tolist() == [255, 0, 255, 0]
    assert set(np.unique(R.source('mask', 40, 40, 0))) == {0, 1} and (R.source('all255', 3, 3, 0) == 255).all()
    sp = R.source('f32_special', 40, 60, 3)
    assert np.isnan(sp).sum() == 1 and np.isposinf(sp).sum() == 1 and np.isneginf(sp).sum() == 1
    assert ((sp == 0) & np.signbit(sp)).sum() == 1
    ys, xs = np.nonzero(~np.isfinite(sp) | (sp == 0))
    assert min(abs(int(ys[i]) - int(ys[j])) + abs(int(xs[i]) - int(xs[j])) for i in range(4) for j in range(i)) >= 20
    assert not np.isnan(R.source('f32_special', 40, 60, 3, 3)).any()
    assert R.source('f32_special', 1, 1, 3).shape == (1, 1)


def test_counts_the_gpu_tests_assert():
    import test_gpu_resize_routes as G
    assert R.planned(R.sweep_items(R.ALL_CODES)) == G.SWEEP_ALL
    assert R.planned(R.sweep_items((R.CUBIC, R.LANCZOS4))) == G.SWEEP_TAPS
    assert R.planned(R.random_items()) == G.RANDOM_ALL
    assert R.planned(R.random_items((R.CUBIC, R.LANCZOS4))) == G.RANDOM_TAPS
    # only INTER_AREA that enlarges is ever skipped
    for items in (R.sweep_items(R.ALL_CODES), R.random_items()):
        for sh, sw, dh, dw, code, kind, skip in items:
            assert skip == (code == R.AREA and (dh > sh or dw > sw))
    # the random cases keep landing on the switch between the forms
    most = [max(R.rows_needed(sh, dh, R.TAPS[code])) for sh, sw, dh, dw, code, kind, skip in R.random_items((R.CUBIC, R.LANCZOS4))]
    assert sum(m == FULL for m in most) >= 5 and sum(m == FULL + 1 for m in most) >= 5
