"""Geometries, sources and the comparison loop of tests/test_gpu_resize_routes.py -- a helper, not a test.

cv.resize with INTER_CUBIC / INTER_LANCZOS4 has two device forms (vkit_amd/csrc/resize.hip): the separable one on 64 x 16
destination tiles, whose source rows sit in LDS (24-row and 40-row instances), and the direct one, a lane a pixel on 64 x 4 tiles.
Which one a call takes depends on the most source rows a 16-row destination tile reaches.  rows_needed() RESTATES that rule --
it neither imports nor parses the library -- so that the geometry lists below can be chosen to sit on both sides of the two
switches (24 | 25 rows, 40 | 41 rows) for either tap count, and tests/test_resize_routes_shapes.py can check on the CPU that
they still do after an edit.

run_sweep() and run_random() compare N.resize with O.resize bit for bit; the GPU tests call them in their own process (default
routing) and, through child_main(), in a child process with VKX_RESIZE_DIRECT=1 (every CUBIC / LANCZOS4 call takes the direct form).
"""
import numpy as np

NEAREST, LINEAR, CUBIC, AREA, LANCZOS4, LINEAR_EXACT, NEAREST_EXACT = range(7)
TAPS = {CUBIC: 4, LANCZOS4: 8}
ALL_CODES = tuple(range(7))
TILE_H = 16            # destination rows of a tile of the separable form


# ---- the row rule ------------------------------------------------------------------------------------------------------

def tap_offsets(ssize, dsize):
    """floor(float32((d + 0.5) * ssize / dsize - 0.5)) for every destination index, as cv.resize states it: the scale is
    1 / (dsize / ssize) in float64 and the coordinate is rounded to float32 before the floor.  (Dividing by dsize last instead
    moves an offset for 26 of the 159 201 size pairs below 400; of the heights in the lists here only for 4 -> 196, the NaN-column
    geometry, where every tap is clipped anyway.)"""
    scale = 1.0 / (float(dsize) / float(ssize))
    f = ((np.arange(dsize, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    return np.floor(f).astype(np.int64)


def tile_rows(sh, dh, ks):
    """[(rows, unclipped)] per 16-row destination tile: the source rows the tile reaches, first tap of its first row to last tap
    of its last row, both clipped to the plane; unclipped: neither end was moved by the clip"""
    yofs = tap_offsets(sh, dh)
    out = []
    for y0 in range(0, dh, TILE_H):
        ylast = min(y0 + TILE_H, dh) - 1
        lo, hi = int(yofs[y0]) - (ks // 2 - 1), int(yofs[ylast]) + ks // 2
        clo, chi = min(max(lo, 0), sh - 1), min(max(hi, 0), sh - 1)
        out.append((chi - clo + 1, clo == lo and chi == hi))
    return out


def rows_needed(sh, dh, ks):
    """the source-row count of every 16-row destination tile of a ks-tap resize of sh rows to dh"""
    return [n for n, _ in tile_rows(sh, dh, ks)]


# ---- the geometries: ((sh, sw), (dh, dw)) --------------------------------------------------------------------------------

BAND_DH = 40                                   # three tiles, the last one of 8 rows
BAND_SW, BAND_DW = 70, 67                      # no multiple of 64 or 4: RGB group stores and the byte tail both run
BANDS = {CUBIC: tuple(range(50, 59)) + tuple(range(93, 102)),
         LANCZOS4: tuple(range(40, 49)) + tuple(range(83, 91))}
# source rows -> the most rows a tile needs at dh = 40; an interior, unclipped tile attains it
CENTRES = {CUBIC: {52: 24, 54: 25, 96: 40, 98: 41},
           LANCZOS4: {42: 24, 44: 25, 85: 40, 86: 41}}
X_EDGE_DW = (63, 64, 65, 66, 67, 127, 129)     # tile and 4-pixel-group edges of both forms in x
X_EDGE_DH = (17, 33)                           # one row into the second and third tile
CLIP = (1, 2, 3, 5, 7)                         # fewer source pixels than taps
NAN_COLUMN = (((146, 4), (64, 196)), ((127, 1), (202, 197)), ((4, 146), (196, 64)))   # LANCZOS4 coefficient 0 / 0 (-32768 on uint8)


def band_geometries(code):
    return [((sh, BAND_SW), (BAND_DH, BAND_DW)) for sh in BANDS[code]]


def transposed_band_geometries(code):
    """the bands along x: the width runs through the band, the height takes the band's fixed sizes"""
    return [((BAND_SW, s), (BAND_DW, BAND_DH)) for s in BANDS[code]]


def x_edge_geometries():
    """destination widths on the tile edges in x, heights one row past a tile in y; a shrink -- 37 -> 17 rows stays with the
    separable form, 82 -> 33 goes to the direct one by itself -- and an enlargement"""
    out = []
    for dw in X_EDGE_DW:
        for dh in X_EDGE_DH:
            out.append(((37 if dh == 17 else 82, 2 * dw - 5), (dh, dw)))
            out.append(((dh // 2 + 2, dw // 2 + 3), (dh, dw)))
    return out


def clipped_geometries():
    """sources of 1, 2, 3, 5, 7 pixels a side, enlarged, shrunk to 1, 2, 3 and mixed"""
    out = []
    n = len(CLIP)
    for i, a in enumerate(CLIP):
        for b in (a, CLIP[(i + 2) % n]):
            out.append(((a, b), (3 * a + 14, 4 * b + 15)))                    # enlarged both ways, past a tile in y
            out.append(((a, b), (1 + i % 3, 1 + (i + 1) % 3)))                # to 1, 2, 3 a side
            out.append(((a, b), (1 + (i + 2) % 3, 70)))                       # a few rows, more than a tile wide
    return out


def scale_geometries():
    """2x and 3.7x, the identity, shrinks by 1.9x, 2.0x (the exact half), 2.1x and 4x"""
    return [((40, 60), d) for d in ((80, 120), (148, 222), (40, 60), (21, 32), (20, 30), (19, 29), (10, 15))]


def near_miss_geometries():
    """the other decisions of the routing rule, just beside their main case"""
    return [((64, 50), (32, 50)), ((64, 66), (32, 32)),       # one axis exactly half, the other not
            ((60, 90), (20, 31)),                             # AREA: integer factor in y only
            ((60, 90), (20, 45)),                             # AREA: unequal integer factors
            ((60, 90), (20, 90)),                             # AREA: factor 1 on one axis
            ((64, 160), (4, 10)),                             # AREA: a large factor
            ((64, 64), (32, 32)),                             # the exact half (float32 LINEAR / LINEAR_EXACT go to AREA)
            ((37, 53), (20, 31)), ((38, 54), (20, 31)), ((37, 54), (61, 83)), ((38, 53), (61, 83))]   # NEAREST_EXACT: odd / even sources


def sweep_geometries():
    """[(geometry, codes it runs with)]: the bands with their own tap count, the x edges with both, the rest with every code"""
    out = []
    for code in (CUBIC, LANCZOS4):
        out += [(g, (code,)) for g in band_geometries(code) + transposed_band_geometries(code)]
    out += [(g, (CUBIC, LANCZOS4)) for g in x_edge_geometries()]
    out += [(g, ALL_CODES) for g in clipped_geometries() + scale_geometries() + list(NAN_COLUMN) + near_miss_geometries()]
    return out


# ---- the sources ---------------------------------------------------------------------------------------------------------

KINDS = ('u8c1', 'u8c3', 'u8c4', 'mask', 'f32', 'all255', 'stripes_x2', 'stripes_x3', 'stripes_x4', 'stripes_y2', 'stripes_y3',
         'stripes_y4', 'f32_special')
SPECIALS = (np.float32(-0.0), np.float32(np.inf), np.float32(-np.inf), np.float32(np.nan))
SPECIAL_LEVELS = (4, 3, 2, 1)       # how many of SPECIALS a plane holds: the first count at which the oracle keeps finite pixels


def _stripes(n, period):
    return np.where(np.arange(n) % period < (period + 1) // 2, 255, 0).astype(np.uint8)


def special_plane(rng, sh, sw, count):
    """random float32 with the first `count` of -0.0, inf, -inf, NaN at the quarter points (fewer where those coincide)"""
    plane = (rng.random((sh, sw), dtype=np.float32) * 80 - 40).astype(np.float32)
    spots = []
    for y, x in ((sh // 4, sw // 4), (3 * sh // 4, 3 * sw // 4), (sh // 4, 3 * sw // 4), (3 * sh // 4, sw // 4)):
        if (y, x) not in spots:
            spots.append((y, x))
    for (y, x), v in zip(spots[:count], SPECIALS):
        plane[y, x] = v
    return plane


def source(kind, sh, sw, seed, special_count=4):
    rng = np.random.default_rng([seed, sh, sw, KINDS.index(kind)])
    if kind in ('u8c1', 'u8c3', 'u8c4'):
        cn = int(kind[-1])
        return rng.integers(0, 256, (sh, sw) if cn == 1 else (sh, sw, cn), dtype=np.uint8)
    if kind == 'mask':
        return (rng.random((sh, sw)) < 0.5).astype(np.uint8)
    if kind == 'f32':
        return (rng.random((sh, sw), dtype=np.float32) * 80 - 40).astype(np.float32)
    if kind == 'all255':
        return np.full((sh, sw, 3), 255, np.uint8)
    if kind.startswith('stripes_x'):           # uint8 extremes: the saturating narrow both ways, RGB along x, 4 channels along y
        return np.ascontiguousarray(np.broadcast_to(_stripes(sw, int(kind[-1]))[None, :, None], (sh, sw, 3)))
    if kind.startswith('stripes_y'):
        return np.ascontiguousarray(np.broadcast_to(_stripes(sh, int(kind[-1]))[:, None, None], (sh, sw, 4)))
    assert kind == 'f32_special', kind
    return special_plane(rng, sh, sw, special_count)


def refused(code, sh, sw, dh, dw):
    """the one combination the library refuses (VkxError): INTER_AREA that enlarges.  (float32 LINEAR / LINEAR_EXACT on the exact
    half go to AREA too, but never enlarge.)"""
    return code == AREA and (dh > sh or dw > sw)


def sweep_items(codes):
    """(sh, sw, dh, dw, code, kind, skip) for every comparison of the sweep restricted to `codes`"""
    for ((sh, sw), (dh, dw)), own in sweep_geometries():
        for code in own:
            if code in codes:
                for kind in KINDS:
                    yield sh, sw, dh, dw, code, kind, refused(code, sh, sw, dh, dw)


RANDOM_SEED, RANDOM_COUNT = 20261019, 8000


def random_items(codes=ALL_CODES, seed=RANDOM_SEED, count=RANDOM_COUNT):
    """`count` seeded cases -- sizes 1 .. 160, a code, a source kind; every second one draws dh from sh / 2.3 .. sh / 1.7, around
    the 40 | 41 row switch between the forms -- of which those with a code in `codes` are returned"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        sh, sw, dh, dw = (int(v) for v in rng.integers(1, 161, 4))
        code = int(rng.integers(0, 7))
        kind = KINDS[int(rng.integers(0, len(KINDS)))]
        band = float(rng.uniform(1.7, 2.3))
        if i % 2:
            dh = max(1, int(round(sh / band)))
        if code in codes:
            out.append((sh, sw, dh, dw, code, kind, refused(code, sh, sw, dh, dw)))
    return out


def planned(items):
    """(comparisons, skipped) of a list of items"""
    items = list(items)
    skipped = sum(1 for it in items if it[6])
    return len(items) - skipped, skipped


# ---- the comparison --------------------------------------------------------------------------------------------------------

def same_bits(got, want):
    """uint8: ==.  float32: equal bit patterns, or NaN on both sides (payloads may differ)"""
    if got.dtype != want.dtype or got.shape != want.shape:
        return None
    if want.dtype == np.float32:
        return (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    return got == want


def oracle_special(O, sh, sw, dh, dw, code, seed):
    """the special-value plane with the most specials whose oracle result is NaN in less than half of the plane, and that result"""
    for count in SPECIAL_LEVELS:
        src = source('f32_special', sh, sw, seed, count)
        want = O.resize(src, (dh, dw), code)
        if 2 * int(np.isnan(want).sum()) < want.size:
            break
    return src, want, count


def compare_items(items, seed=0):
    """Runs every item on the device and on the oracle.  Returns (compared, skipped, failures): failures are strings, one per
    comparison that differs or that was not refused as it should be."""
    from vkit_amd import _native as N
    import oracle as O
    compared = skipped = 0
    failures = []
    for sh, sw, dh, dw, code, kind, skip in items:
        tag = f'code {code} {kind} ({sh}, {sw}) -> ({dh}, {dw})'
        if skip:
            try:
                N.resize(source(kind, sh, sw, seed), (dh, dw), code)
                failures.append(f'{tag}: INTER_AREA enlarging was not refused')
            except N.VkxError:
                pass
            skipped += 1
            continue
        if kind == 'f32_special':
            src, want, count = oracle_special(O, sh, sw, dh, dw, code, seed)
            if not 2 * int(np.isnan(want).sum()) < want.size:
                failures.append(f'{tag}: the oracle is NaN in {int(np.isnan(want).sum())} of {want.size} pixels with {count} special(s)')
        else:
            src = source(kind, sh, sw, seed)
            want = O.resize(src, (dh, dw), code)
        got = np.asarray(N.resize(src, (dh, dw), code))
        same = same_bits(got, want)
        compared += 1
        if same is None:
            failures.append(f'{tag}: {got.dtype} {got.shape} != {want.dtype} {want.shape}')
        elif not same.all():
            idx = np.argwhere(~same)
            first = tuple(int(v) for v in idx[0])
            failures.append(f'{tag}: {idx.shape[0]} values differ, rows {int(idx[:, 0].min())} .. {int(idx[:, 0].max())}, '
                            f'first at {first}: {got[first]!r} != {want[first]!r}')
    return compared, skipped, failures


def _checked(compared, skipped, failures):
    assert not failures, f'{len(failures)} of {compared + skipped} resize cases differ from the oracle:\n' + '\n'.join(failures[:40])
    return compared, skipped


def run_sweep(codes):
    """the geometry lists x `codes` x the sources, each compared bit for bit: (comparisons made, skipped)"""
    return _checked(*compare_items(sweep_items(codes), seed=1))


def run_random(codes=ALL_CODES):
    """the seeded random cases with a code in `codes`: (comparisons made, skipped)"""
    return _checked(*compare_items(random_items(codes), seed=2))


SENTINEL = 'resize routes child:'


def child_main():
    """what the forced-direct child process runs: the sweep and the random cases of CUBIC and LANCZOS4, then one report line
    {part: [compared, skipped, seconds] or the failures' text}"""
    import json
    import os
    import time
    assert os.environ.get('VKX_RESIZE_DIRECT'), 'the child is meant to run with VKX_RESIZE_DIRECT set'
    report = {}
    for name, fn in (('sweep', run_sweep), ('random', run_random)):
        t0 = time.perf_counter()
        try:
            report[name] = list(fn((CUBIC, LANCZOS4))) + [round(time.perf_counter() - t0, 2)]
        except AssertionError as e:
            report[name] = str(e)
    print(SENTINEL, json.dumps(report))
