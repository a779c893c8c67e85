#!/usr/bin/env python3
"""Times the external_ellipse char labels of one page: the device call against the numpy + oracle restatement.

    python tools/char_mask.py [--size 1024] [--chars 1000] [--side 40] [--calls 20] [--out FILE]

The page's three ellipse sets -- char mask, seal-impression char mask (chars / 20) and char height map -- go through ONE
vkx_char_mask_ellipse_sets_fresh_dev call, as PageDistortionStep makes it on a device-resident page.  Prints one JSON
object: kernel time per launch (the context's timing table), launches per call, device time per page (kernels summed) and
host time per call, next to the restatement's time per page (tests/char_mask_restate.py, one char after the other as the
reference runs it)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
from numpy.random import default_rng  # noqa: E402


def page_quads(size, n, seed=0):
    """n chars of 4 .. 40 px side over a size^2 page, rotated and in mild perspective, clear of the edges."""
    rng = default_rng(seed)
    side = rng.uniform(4, 40, n)
    centre = rng.uniform(48, size - 48, (n, 2))
    a = rng.uniform(-0.5, 0.5, n)
    rot = np.stack([np.stack([np.cos(a), -np.sin(a)], 1), np.stack([np.sin(a), np.cos(a)], 1)], 1)
    base = np.array([(-1, -1), (1, -1), (1, 1), (-1, 1)], np.float64)[None] * (side[:, None, None] / 2)
    q = np.einsum('nij,nkj->nki', rot, base) + rng.uniform(-0.1, 0.1, (n, 4, 2)) * side[:, None, None]
    return np.round(q + centre[:, None, :], 3), side + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--chars', type=int, default=1000)
    ap.add_argument('--side', type=int, default=40)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--restate-chars', type=int, default=200, help='chars timed through the restatement (per-char cost)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'char_mask_kernels.json'))
    args = ap.parse_args()

    from vkit_amd import _native as N
    import char_mask_restate as R
    ctx = N.default_ctx()
    size = args.size
    chars, heights = page_quads(size, args.chars)
    seal, _ = page_quads(size, max(1, args.chars // 20), seed=1)
    order = np.argsort(heights)[::-1]

    def call():
        sets = [N.CharMaskSet(chars, mask=ctx.dev_empty((size, size), np.uint8)),
                N.CharMaskSet(seal, mask=ctx.dev_empty((size, size), np.uint8)),
                N.CharMaskSet(chars[order], values=heights[order], score=ctx.dev_empty((size, size), np.float32))]
        assert N.char_mask_ellipse_sets(args.side, sets, (size, size))
        return sets

    sets = call()
    want, _ = R.run(chars[:50], args.side, (size, size))       # a spot check of the first chars' union on their own
    ctx.sync()
    ctx.set_timing(1)
    ctx.reset_timings()
    t0 = time.perf_counter()
    for _ in range(args.calls):
        call()
    ctx.sync()
    host_ms = (time.perf_counter() - t0) * 1e3 / args.calls
    timings = ctx.timings()
    ctx.set_timing(0)
    kernels = {name: {'us_per_launch': round(ms * 1e3 / n, 2), 'launches_per_call': n / args.calls}
               for name, (ms, n) in sorted(timings.items()) if name.startswith('k_char_mask')}
    device_us = sum(ms for name, (ms, n) in timings.items() if name.startswith('k_char_mask')) * 1e3 / args.calls
    # the same call timed without events (the event pairs cost stream time of their own)
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(args.calls):
        call()
    ctx.sync()
    untimed_ms = (time.perf_counter() - t0) * 1e3 / args.calls

    k = min(args.restate_chars, args.chars)
    t0 = time.perf_counter()
    R.run(chars[:k], args.side, (size, size))
    restate_ms_per_char = (time.perf_counter() - t0) * 1e3 / k
    n_total = 2 * args.chars + len(seal)
    result = {
        'page': [size, size], 'chars': args.chars, 'seal_chars': len(seal), 'internal_side_length': args.side,
        'sets_per_call': 3, 'char_entries_per_call': n_total,
        'kernels': kernels,
        'kernel_us_per_page': round(device_us, 2),
        'host_ms_per_call': round(host_ms, 3),
        'host_ms_per_call_untimed': round(untimed_ms, 3),
        'syncs_per_call': 1,
        'restatement_ms_per_char': round(restate_ms_per_char, 4),
        'restatement_ms_per_page_estimate': round(restate_ms_per_char * n_total, 1),
        'spot_check_union_pixels': int(want.sum()),
        'vkx_version': N.lib().vkx_version(),
    }
    assert (sets[0].mask.host()[want > 0] == 1).all()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
