#!/usr/bin/env python3
"""Times TextRegionFlattener.get_bounding_extended_text_region_masks on one page: the method in resident mode against the
numpy + oracle restatement on the same polygons.

    python tools/text_region_masks.py [--size 1024] [--regions 70] [--calls 20] [--out FILE]

The page holds ``--regions`` random quadrilateral regions (tests/text_region_masks_restate.py random_region, scaled to the
page: 40 .. 280 px long), every second one typical.  Prints one JSON object: kernel time per call of every kernel the method
runs (the context's timing table, HIP events around each launch), launches per call, the host time of a call (queueing only:
the method does not synchronise) and of a call followed by a stream drain, and the wall time of the restatement, which runs one
region after the other on the host as the reference does.  The method's masks must equal the restatement's."""
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
    ap.add_argument('--regions', type=int, default=70)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'text_region_masks_kernels.json'))
    args = ap.parse_args()

    from vkit_amd import _native as N
    from vkit_amd.element import Polygon
    from vkit_amd.pipeline.text_detection import TextRegionFlattener
    import text_region_masks_restate as R
    ctx = N.default_ctx()
    shape = (args.size, args.size)
    rng = default_rng(0)
    scale = 10.0
    small = (int(args.size / scale), int(args.size / scale))
    regions = []
    for _ in range(args.regions):
        regions.append(tuple(R.clip(points * scale, shape) for points in R.random_region(rng, small)))
    angles = [R.ANGLES[k % len(R.ANGLES)] for k in range(args.regions)]
    typical = list(range(0, args.regions, 2))

    def polygon_of(points):
        return Polygon.from_xy_pairs([(int(x), int(y)) for x, y in points])

    originals = [polygon_of(o) for o, _, _ in regions]
    dilated = [polygon_of(d) for _, d, _ in regions]
    given = [polygon_of(r) for _, _, r in regions]
    rectangles = [r if k in typical else np.array([(p.x, p.y) for p in dilated[k].to_bounding_rectangular_polygon(shape, angles[k]).points], np.int32)
                  for k, (_, _, r) in enumerate(regions)]

    def call():
        return TextRegionFlattener.get_bounding_extended_text_region_masks(shape, originals, dilated, given, typical, angles)

    def restate():
        return R.extended_masks(shape, [o for o, _, _ in regions], [d for _, d, _ in regions], rectangles)

    with N.resident(True):
        got = call()
        want = restate()
        for mask, (mat, box) in zip(got, want):
            assert (mask.box.up, mask.box.down, mask.box.left, mask.box.right) == box and mask.mat.tobytes() == mat.tobytes()
        pixels = sum(mat.size for mat, _ in want)
        for _ in range(3):
            call()
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            call()
        queue_ms = (time.perf_counter() - t0) * 1e3 / args.calls
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            call()
            ctx.sync()
        drained_ms = (time.perf_counter() - t0) * 1e3 / args.calls
        ctx.set_timing(1)
        ctx.reset_timings()
        for _ in range(args.calls):
            call()
        timings = ctx.timings()
        ctx.set_timing(0)
    t0 = time.perf_counter()
    reps = 3
    for _ in range(reps):
        restate()
    restate_ms = (time.perf_counter() - t0) * 1e3 / reps
    kernels = {name: dict(ms_per_call=ms / args.calls, launches_per_call=cnt / args.calls) for name, (ms, cnt) in sorted(timings.items())}
    result = dict(what='get_bounding_extended_text_region_masks, one %d x %d page, %d regions, resident mode' % (shape + (args.regions,)),
                  region_box_pixels=pixels, calls=args.calls, kernels=kernels,
                  kernel_ms_per_call=sum(k['ms_per_call'] for k in kernels.values()),
                  host_ms_per_call_queued=queue_ms, host_ms_per_call_drained=drained_ms,
                  restatement_numpy_ms_per_call=restate_ms,
                  note='kernel times: HIP events around every launch (vkx_ctx_collect_timings), the paint of the text mask included; '
                       'host times: perf_counter around the Python method, polygon objects to Masks; the restatement: numpy over the '
                       'oracle fill_poly in C, one region after the other, one CPU thread')
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
