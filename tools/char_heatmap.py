#!/usr/bin/env python3
"""Times the default char heatmap of one page: the device call against the numpy + oracle restatement.

    python tools/char_heatmap.py [--size 1024] [--chars 1000] [--calls 20] [--debug] [--out FILE]

The page holds ``--chars`` chars laid out as touching and overlapping text lines (tests/char_heatmap_restate.py
text_line_quads).  The engine runs on a device-resident page (one vkx_char_heatmap_fresh_dev call).  Prints one JSON
object: kernel time per launch (the context's timing table), launches per call, device time per page (kernels summed),
host time per call with and without the timing events, the Context.sync calls per call, and the restatement's time per
char (one char after the other as the reference runs it).  The result must equal the restatement bit for bit."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--chars', type=int, default=1000)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--debug', action='store_true', help='also write the six debug planes')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'char_heatmap_kernels.json'))
    args = ap.parse_args()

    from vkit_amd import _native as N
    from vkit_amd.element import PolygonSoup
    from vkit_amd.engine.char_heatmap import char_heatmap_default_engine_executor_factory as F
    import char_heatmap_restate as R
    ctx = N.default_ctx()
    shape = (args.size, args.size)
    quads = R.text_line_quads(default_rng(0), shape, args.chars, step=(0.75, 1.0))
    soup = PolygonSoup(np.ascontiguousarray(quads.reshape(-1, 2)), np.arange(0, 4 * len(quads) + 1, 4, dtype=np.int64))
    executor = F.create()
    run_config = {'height': shape[0], 'width': shape[1], 'char_polygons': soup, 'enable_debug': args.debug}

    def call():
        with N.resident(True):
            return executor.run(run_config)

    out = call()
    want = R.run(quads, shape)
    assert out.score_map.mat.tobytes() == want['score'].tobytes()
    ctx.sync()
    syncs = []
    real_sync = N.Context.sync
    N.Context.sync = lambda self: syncs.append(1) or real_sync(self)
    try:
        ctx.set_timing(1)
        ctx.reset_timings()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            call()
        host_ms = (time.perf_counter() - t0) * 1e3 / args.calls
        syncs_per_call = len(syncs) / args.calls
    finally:
        N.Context.sync = real_sync
    ctx.sync()
    timings = ctx.timings()
    ctx.set_timing(0)
    kernels = {name: {'us_per_launch': round(ms * 1e3 / n, 2), 'launches_per_call': n / args.calls}
               for name, (ms, n) in sorted(timings.items()) if name.startswith('k_char_heatmap')}
    device_us = sum(ms for name, (ms, n) in timings.items() if name.startswith('k_char_heatmap')) * 1e3 / args.calls
    # the same calls without events (an event pair costs stream time of its own); wall time per call with the stream drained
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(args.calls):
        call()
    ctx.sync()
    untimed_ms = (time.perf_counter() - t0) * 1e3 / args.calls

    t0 = time.perf_counter()
    R.run(quads, shape)
    restate_ms_per_char = (time.perf_counter() - t0) * 1e3 / len(quads)
    result = {
        'page': list(shape), 'chars': len(quads), 'layout': 'text lines, advance 0.75 .. 1.0 of the char width',
        'radius': 25, 'debug_planes': bool(args.debug),
        'kernels': kernels,
        'launches_per_call': sum(v['launches_per_call'] for v in kernels.values()),
        'kernel_us_per_page': round(device_us, 2),
        'host_ms_per_call': round(host_ms, 3),
        'wall_ms_per_call_untimed': round(untimed_ms, 3),
        'syncs_per_call': syncs_per_call,
        'restatement_ms_per_char': round(restate_ms_per_char, 4),
        'restatement_ms_per_page': round(restate_ms_per_char * len(quads), 1),
        'overlapped_pixels': int(want['char_overlapped_mask'].sum()),
        'neutralized_pixels': int(want['neutralized_mask'].sum()),
        'vkx_version': N.lib().vkx_version(),
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
