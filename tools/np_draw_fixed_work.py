#!/usr/bin/env python3
"""Where the VALU instructions of k_np_draw_compact<EmitI16> go per tile: the static count of every basic block
(tools/np_draw_census.py) weighted by how often the block runs per tile.

How often comes from a CPU-side count over numpy's own raw stream (PCG64 random_raw; the draw pass's tables from np_ziggurat.h):
per tile of 3 072 draws the events (draws whose attempt is not a fast accept), the rounds that push one, whether any event of the
tile's first 64 is a tail draw and how many passes the tail loop makes, whether any wedge test needs the float64 exp(), the
events some earlier span reaches, the phase-3 walks and the cover loop's trips.  Blocks are sorted into the kernel's parts by what
they hold (tools/np_draw_census.py's block split; the rules are below in `part_of`); a part's blocks run as often as the part.

Usage: tools/np_draw_fixed_work.py [--src nprand.hip] [--run-carry] [--jobs 16] [--tiles-per-wave 2] [--tiles 3000] [--scale 10]
                                   [--valu SQ_INSTS_VALU] [--waves SQ_WAVES]
  --jobs / --tiles-per-wave / --valu / --waves: the launch the PMC figures were taken at (bench --batch 32: two launches of 16
  streams per step, ~78 700 tiles each, two tiles per wavefront).  Tiles per launch = wavefronts x tiles per wavefront: the
  streams are the noise planes of the distorted images (4.85 Mpixel on average, not 2048^2), ~4 800 tiles each."""
import argparse
import math
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_draw_census as C   # noqa: E402

ROOT = C.ROOT
ROUNDS, TILE = 48, 3072


def tables():
    text = open(os.path.join(ROOT, 'vkit_amd', 'csrc', 'np_ziggurat.h')).read()
    out = {}
    for name in ('kNpZigK', 'kNpZigW', 'kNpZigF'):
        body = re.search(name + r'\[256\]\s*=\s*\{(.*?)\}', text, re.S).group(1)
        out[name] = np.array([int(v.strip().rstrip('uUlL'), 0) for v in body.split(',') if v.strip()], np.uint64)
    return out['kNpZigK'], out['kNpZigW'].view(np.float64), out['kNpZigF'].view(np.float64)


def u2dbl(u):
    return (u >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


TAIL_EPS = 2.0 ** -16      # kTailEps of nprand.hip
K_INV_R, NOR_R = 0.27366123732975827, 3.6541528853610088


def tail_fast_pass(u1, u2, neg, scale):
    """The fast tail pass of the integer emitters as nprand.hip decides it, with numpy's float32 log2 standing in for v_log_f32:
    'reject' / 'accept' when the float32 estimates prove the pass (and, for an accept, the emitted integer), else 'float64'."""
    l1 = -0.6931471805599453 * float(np.log2(np.float32(1.0 - u1)))
    l2 = -0.6931471805599453 * float(np.log2(np.float32(1.0 - u2)))
    xe = K_INV_R * l1
    r2 = xe * xe
    diff = 2.0 * l2 - r2
    bound = 2.0 * TAIL_EPS + K_INV_R * K_INV_R * (2.0 * l1 * TAIL_EPS + TAIL_EPS * TAIL_EPS) + 2.0 ** -30 * (1.0 + r2)
    if abs(diff) <= bound:
        return 'float64'
    if diff < 0.0:
        return 'reject'
    v = scale * (-(NOR_R + xe) if neg else NOR_R + xe)
    dist = abs((v - math.floor(v)) - 0.5)
    return 'accept' if dist > abs(scale) * K_INV_R * TAIL_EPS + 2.0 ** -26 + abs(v) * 2.0 ** -50 else 'float64'


def tile_stats(n_tiles, seed, scale=10.0, fast_tail=True):
    """Per tile: events, push rounds, tail passes of the first phase-2 pass, exp() fallback, reach / touch, cover-loop trips."""
    ki, wi, fi = tables()
    raw = np.random.default_rng(seed).bit_generator.random_raw(n_tiles * TILE + 512).astype(np.uint64)
    idx = (raw & np.uint64(0xff)).astype(np.int64)
    rabs = (raw >> np.uint64(9)) & np.uint64((1 << 52) - 1)
    slow = rabs >= ki[idx]
    st = {k: [] for k in ('nev', 'push_rounds', 'tail_passes', 'tail_f64', 'tail_all', 'exp_any', 'touch', 'reach', 'cov_trips', 'over64')}
    for t in range(n_tiles):
        b = t * TILE
        pos = np.flatnonzero(slow[b:b + TILE])
        nev = len(pos)
        st['nev'].append(nev)
        st['over64'].append(nev > 64)
        st['push_rounds'].append(len(np.unique(pos >> 6)))
        lens, exp_any, passes, f64, all_passes = [], False, 0, 0, 0
        for k, p in enumerate(pos):
            g = b + p
            if idx[g] != 0:
                lens.append(2)
                if k < 64:
                    x = float(rabs[g]) * wi[idx[g]]
                    un = u2dbl(raw[g + 1:g + 2])[0]
                    lhs = (fi[idx[g] - 1] - fi[idx[g]]) * un + fi[idx[g]]
                    r32 = np.float32(np.exp2(np.float32(-0.5 * x * x) * np.float32(1.44269504)))
                    exp_any |= abs(np.float32(lhs) - r32) <= r32 * np.float32(2.0 ** -14)
            else:
                n, q = 1, g
                while True:
                    u1, u2 = u2dbl(raw[q + 1:q + 3])
                    q += 2
                    n += 2
                    all_passes += 1
                    # (a trip of the tail loop runs the float64 pass when one of its lanes asks for it: rare enough to add up)
                    if fast_tail and k < 64 and tail_fast_pass(u1, u2, (int(rabs[g]) >> 8) & 1, scale) == 'float64':
                        f64 += 1
                    xx = -0.27366123732975827 * math.log1p(-u1)
                    if -2 * math.log1p(-u2) > xx * xx:
                        break
                lens.append(n)
                if k < 64:
                    passes = max(passes, (n - 1) // 2)
        st['tail_passes'].append(passes)
        st['tail_f64'].append(f64 if fast_tail else passes)
        st['tail_all'].append(all_passes)
        st['exp_any'].append(exp_any)
        ends = pos + np.array(lens, np.int64)
        prev_end = np.concatenate(([0], ends[:-1]))
        touch = bool((pos < prev_end).any())
        st['touch'].append(touch)
        run_max = np.maximum.accumulate(np.concatenate(([0], ends[:-1]))) if nev else np.zeros(0, np.int64)
        st['reach'].append(int((pos < run_max).sum()) if touch else 0)
        # valid events and the chunks of 64 draws their spans cover (one trip of the cover loop per chunk, lanes in parallel)
        cover, trips = 0, 0
        for p, e in zip(pos, ends):
            if p >= cover:
                cover = e
                lo, hi = p + 1, min(e, TILE)
                trips = max(trips, ((hi - 1) >> 6) - (lo >> 6) + 1 if hi > lo else 0)
        st['cov_trips'].append(trips)
    return {k: np.array(v, np.float64) for k, v in st.items()}


def part_of(b, phase1_loop, loops):
    """The kernel part a block belongs to (tile-loop structure of k_np_draw_compact; see the module docstring)."""
    if b['depth'] == 0:
        return 'per wavefront'
    if b['loop'] == phase1_loop:
        return 'phase 1 push' if C.is_push(b) else 'phase 1'
    if b['depth'] >= 2:
        sig = loops[b['loop']]
        if sig['rcp']:
            # (a build with the fast tail pass keeps the float64 pass -- the blocks with log1p's divisions -- for the lanes in doubt)
            return 'tail float64 pass' if sig['log32'] and any(o.startswith('v_rcp_f64') for o in b['ops']) else 'tail loop'
        if sig['gload']:
            return 'job search'
        if sig['readlane'] and not sig['ds']:
            return 'phase 3 walk'
        if sig['depth3'] or sig['ds_read_u16']:
            return 'phase 3 serial (> 64 events)'
        if sig['lshl64']:
            return 'phase 3 cover loop'
        return 'other loop'
    return 'per tile'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--src', default=os.path.join(ROOT, 'vkit_amd', 'csrc', 'nprand.hip'))
    ap.add_argument('--jobs', type=int, default=16)
    ap.add_argument('--tiles-per-wave', type=float, default=2)
    ap.add_argument('--tiles', type=int, default=3000)
    ap.add_argument('--seed', type=int, default=12345)
    ap.add_argument('--scale', type=float, default=10.0, help='std of the streams (the bench draws at 10): the fast tail pass proves its integer against it')
    ap.add_argument('--valu', type=float, default=2.2452e8, help='PMC SQ_INSTS_VALU of k_np_draw_compact per launch')
    ap.add_argument('--waves', type=float, default=39364, help='PMC SQ_WAVES of the same launches')
    ap.add_argument('--run-carry', action='store_true', help='the build carries the lane states along a run of tiles')
    args = ap.parse_args()
    rates = C.load_rates()
    blocks = C.kernel_blocks(C.compile_asm(args.src, []))
    mads = {}
    for b in blocks:
        if b['depth'] == 2:
            mads[b['loop']] = mads.get(b['loop'], 0) + b['ops'].count('v_mad_u64_u32')
    phase1 = max(mads, key=mads.get)
    loops = {}
    for b in blocks:
        if b['depth'] >= 2:
            s = loops.setdefault(b['loop'], {'rcp': False, 'log32': False, 'gload': False, 'readlane': False, 'ds': False, 'depth3': False,
                                             'ds_read_u16': False, 'lshl64': False})
            s['rcp'] |= any(o.startswith('v_rcp_f64') for o in b['ops'])
            s['log32'] |= any(o.startswith('v_log_f32') for o in b['ops'])
            s['gload'] |= any(o.startswith('global_load') for o in b['ops'])
            s['readlane'] |= 'v_readlane_b32' in b['ops']
            s['ds'] |= any(o.startswith('ds_') for o in b['ops'])
            s['depth3'] |= b['depth'] >= 3
            s['ds_read_u16'] |= 'ds_read_u16' in b['ops']
            s['lshl64'] |= 'v_lshlrev_b64' in b['ops']
    # phase 2 runs in passes of 64 events (two copies in the code): the second only when a tile has more than 64 events.  Within a
    # pass the float64 exp() fallback (the depth-1 block with v_fma_f64 after the one with v_exp_f32) runs when a lane asks for
    # it, the tail branch around its loop (the block before the loop and those after it up to the mask atomics) when a lane has one
    parts = [part_of(b, phase1, loops) for b in blocks]
    tail_idx = [i for i, p in enumerate(parts) if p in ('tail loop', 'tail float64 pass')]
    cond = {}
    if tail_idx:
        heads = sorted({blocks[i]['loop'] for i in tail_idx}, key=lambda l: min(i for i in tail_idx if blocks[i]['loop'] == l))
        spans = [(min(i for i in tail_idx if blocks[i]['loop'] == l), max(i for i in tail_idx if blocks[i]['loop'] == l)) for l in heads]
        def atomics_after(i):
            j = i + 1
            while j < len(blocks) and 'ds_or_b64' not in blocks[j]['ops']:
                j += 1
            while j + 1 < len(blocks) and 'ds_or_b64' in blocks[j + 1]['ops']:
                j += 1
            return j
        exps = [i for i, b in enumerate(blocks) if 'v_exp_f32_e32' in b['ops'] and parts[i] == 'per tile']
        for k, (a, z) in enumerate(spans):
            e = atomics_after(z)
            cond[a - 1] = 'tail branch'
            for i in range(z + 1, e):
                cond[i] = 'tail branch'
            if k == 1:
                start = atomics_after(spans[0][1]) + 1
                for i in range(start, e + 2):
                    cond[i] = 'phase 2, second pass'
        for i in exps:
            j = i + 1
            while 'v_fma_f64' not in blocks[j]['ops']:
                j += 1
            if cond.get(j) != 'phase 2, second pass':
                cond[j] = 'exp() fallback'
    for i, c in cond.items():
        if parts[i] in ('per tile',) or c == 'phase 2, second pass':
            parts[i] = c
    # the tile start (the lane states from the tile's state: the block with the 128-bit products outside phase 1) and, where the
    # build has it, the max-scan of phase 3 (DPP row broadcasts; it runs in the tiles where two events touch)
    # depth-1 blocks of another loop than the tile loop (the table load) run once per wavefront; the compaction is the block with
    # the most v_readlane; the wedge tests of phase 2 are the per-tile blocks between phase 1 and the first tail loop
    tile_loop = max({b['loop'] for b in blocks if b['depth'] == 1}, key=lambda l: sum(b['loop'] == l for b in blocks))
    comp = max(range(len(blocks)), key=lambda i: blocks[i]['ops'].count('v_readlane_b32'))
    last_p1 = max(i for i, p in enumerate(parts) if p.startswith('phase 1'))
    for i, b in enumerate(blocks):
        if parts[i] == 'per tile' and b['loop'] != tile_loop:
            parts[i] = 'per wavefront'
        elif i == comp:
            parts[i] = 'compaction'
        elif parts[i] == 'per tile' and tail_idx and last_p1 < i < tail_idx[0]:
            parts[i] = 'phase 2 wedge pass'
    for i, b in enumerate(blocks):
        if parts[i] == 'per tile' and b['ops'].count('v_mad_u64_u32') >= 8:
            parts[i] = 'tile start'
        elif parts[i] == 'per tile' and any('row_bcast' in s for s in b.get('text', [])):
            parts[i] = 'phase 3 reach scan'
    fast_tail = any(s['log32'] for s in loops.values())
    st = tile_stats(args.tiles, args.seed, args.scale, fast_tail)
    k1 = sum(b['ops'].count('ds_read_b128') for b in blocks if b['loop'] == phase1 and not C.is_push(b)) or 2
    trips = ROUNDS / k1
    # per tile: how often a block of each part runs
    freq = {
        'per wavefront': 1.0 / args.tiles_per_wave,
        'per tile': 1.0,
        'compaction': 1.0,
        'phase 2 wedge pass': 1.0,
        # a run of tiles starts once per wavefront (a new job inside a run adds at most one start per job and launch: < 0.1 %)
        'tile start': 1.0 / args.tiles_per_wave if args.run_carry else 1.0,
        'phase 3 reach scan': float(st['touch'].mean()),
        'phase 1': trips,
        'phase 1 push': None,            # a push block belongs to one round of the trip: it runs when that round has an event
        'job search': math.ceil(math.log2(max(args.jobs, 2))) / (args.tiles_per_wave if args.run_carry else 1.0),
        'tail loop': float(st['tail_passes'].mean()),
        'tail float64 pass': float(st['tail_f64'].mean()),
        'phase 3 walk': float((st['reach'] if args.run_carry else st['nev'] * st['touch']).mean()),
        'phase 3 serial (> 64 events)': float((st['nev'] * st['over64']).mean()),
        'phase 3 cover loop': float(st['cov_trips'].mean()),
        'other loop': 1.0,
        'tail branch': float((st['tail_passes'] > 0).mean()),
        'exp() fallback': float(st['exp_any'].mean()),
        'phase 2, second pass': float(st['over64'].mean()),
    }
    push_frac = float(np.mean(st['push_rounds'])) / ROUNDS     # rounds with an event
    rows = {}
    for b, part in zip(blocks, parts):
        c, _ = C.summarize(b, rates)
        f = freq[part] if part != 'phase 1 push' else push_frac * trips
        rows.setdefault(part, [0, 0.0, []])
        rows[part][0] += c['valu']
        rows[part][1] += c['valu'] * f
        if c['valu']:
            rows[part][2].append(b['name'])
    total = sum(r[1] for r in rows.values())
    print(f'# k_np_draw_compact<EmitI16>: VALU per tile by part ({os.path.relpath(args.src, ROOT)})\n')
    print(f'CPU-side count over {args.tiles} tiles of numpy\'s raw stream (seed {args.seed}): events per tile '
          f'{st["nev"].mean():.1f}, rounds with an event {push_frac:.3f}, tiles with a tail pass {np.mean(st["tail_passes"] > 0):.3f} '
          f'(passes {st["tail_passes"].mean():.3f}), exp() fallback {st["exp_any"].mean():.4f}, touch {st["touch"].mean():.3f}, '
          f'events an earlier span reaches {st["reach"].mean():.2f}, > 64 events {st["over64"].mean():.4f}.  '
          f'Launch: {args.jobs} streams, {args.tiles_per_wave:g} tiles per wavefront.\n')
    if fast_tail:
        print(f'Fast tail pass (std {args.scale:g}): {int(st["tail_all"].sum())} tail passes in all, {int(st["tail_f64"].sum())} of them through the '
              f'float64 pass ({100 * st["tail_f64"].sum() / max(1.0, st["tail_all"].sum()):.3f} %).\n')
    print('| part | blocks | static VALU | runs per tile | VALU per tile | per round |')
    print('|---|---|---|---|---|---|')
    for part, (v, w, names) in sorted(rows.items(), key=lambda kv: -kv[1][1]):
        f = w / v if v else 0.0
        shown = ', '.join(names[:4]) + (f', +{len(names) - 4}' if len(names) > 4 else '')
        print(f'| {part} | {shown} | {v} | {f:.3f} | {w:.0f} | {w / ROUNDS:.1f} |')
    print(f'| **sum** | | | | **{total:.0f}** | **{total / ROUNDS:.1f}** |')
    # the launch grid is ceil(tiles / (8 x tiles per wavefront)) workgroups of 8 wavefronts: tiles = waves x tiles per wavefront,
    # less than 8 x tiles-per-wavefront short of it
    pmc = args.valu / (args.waves * args.tiles_per_wave) / ROUNDS
    print(f'\nPMC: SQ_INSTS_VALU {args.valu:.5g} over {args.waves:.0f} wavefronts of {args.tiles_per_wave:g} tiles = {pmc:.1f} per round '
          f'({pmc * ROUNDS:.0f} per tile); the model: {total / ROUNDS:.1f} ({100 * (total / ROUNDS / pmc - 1):+.1f} %).')


if __name__ == '__main__':
    sys.exit(main())
