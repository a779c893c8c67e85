#!/usr/bin/env python3
"""Times Mask.fill_by_polygons on one device-resident mask against the same work written without it: a loop of
Polygon.fill_mask.

    python tools/element_sets.py [--size 1024] [--polygons 200] [--runs 30] [--out FILE]

The list is ``--polygons`` text-line-like quads (tests/element_sets_restate.py quads, scaled to the page).  Four forms, each run
ending in a stream synchronisation, timed with the host clock in alternation, medians over ``--runs`` runs after 5 warm-up runs:

  batched        mask.fill_by_polygons(polygons)                       one set-mask call + one composite call
  batched,       the same over Polygon objects that exist already      (their cached rasters are not used)
  prebuilt
  loop, fresh    for p in polygons: p.fill_mask(mask)                  polygons built anew: one raster launch, one download and
                                                                       one composite call a polygon
  loop, cached   the same loop over polygons whose np_mask is cached   one composite call (with a host mask plane) a polygon

Also the launches of a batched run (the context's timing table).  All must leave the same mask.  Prints one JSON object."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--polygons', type=int, default=200)
    ap.add_argument('--runs', type=int, default=30)
    ap.add_argument('--out', default='')
    ap.add_argument('--profile', default='', help='write a cProfile listing of 20 batched runs to this file')
    args = ap.parse_args()

    from vkit_amd import _native as N
    from vkit_amd.element import Mask, Polygon
    import element_sets_restate as R
    ctx = N.default_ctx()
    shape = (args.size, args.size)
    scale = args.size // 256
    tables = [np.array(q, np.int32) * scale for q in R.quads(np.random.default_rng(2024), (256, 256), args.polygons)]

    def build():
        return [Polygon.from_xy_pairs([(int(x), int(y)) for x, y in t]) for t in tables]

    cached = build()
    for polygon in cached:
        polygon.np_mask

    def batched(polygons=None):
        mask = Mask(mat=N.dev_zeros(shape, np.uint8, ctx))
        mask.fill_by_polygons(polygons or build())
        return mask

    def loop(polygons):
        mask = Mask(mat=N.dev_zeros(shape, np.uint8, ctx))
        for polygon in polygons:
            polygon.fill_mask(mask)
        return mask

    forms = {'batched': batched, 'batched_prebuilt': lambda: batched(cached), 'loop_fresh': lambda: loop(build()),
             'loop_cached': lambda: loop(cached)}
    want = R.set_mask(R.POLYGONS, tables, shape, 'union')
    for name, form in forms.items():
        assert form().mat.tobytes() == want.tobytes(), name
    times = {name: [] for name in forms}
    for run in range(5 + args.runs):
        for name, form in forms.items():
            ctx.sync()
            t0 = time.perf_counter()
            form()
            ctx.sync()
            if run >= 5:
                times[name].append((time.perf_counter() - t0) * 1e3)
    if args.profile:
        import cProfile
        import io
        import pstats
        profile = cProfile.Profile()
        profile.enable()
        for _ in range(20):
            batched()
        ctx.sync()
        profile.disable()
        listing = io.StringIO()
        pstats.Stats(profile, stream=listing).sort_stats('cumulative').print_stats(45)
        with open(args.profile, 'w') as f:
            f.write(listing.getvalue())
    ctx.set_timing(1)
    ctx.reset_timings()
    batched()
    timings = ctx.timings()
    ctx.set_timing(0)
    result = dict(what='Mask.fill_by_polygons, %d quads, device-resident %d x %d mask, UNION' % ((args.polygons,) + shape),
                  runs=args.runs,
                  median_ms={name: statistics.median(v) for name, v in times.items()},
                  min_ms={name: min(v) for name, v in times.items()},
                  max_ms={name: max(v) for name, v in times.items()},
                  batched_launches={name: cnt for name, (_ms, cnt) in sorted(timings.items())},
                  batched_kernel_ms={name: ms for name, (ms, _cnt) in sorted(timings.items())},
                  note='host clock around the Python call and a stream synchronisation; the Polygon objects are built inside the '
                       'timed window of batched and loop_fresh, not of batched_prebuilt and loop_cached')
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
