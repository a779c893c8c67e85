#!/usr/bin/env python3
"""Times PageTextRegionLabelStep on one page: the step on a device-resident page against the numpy + oracle restatement.

    python tools/text_region_label.py [--size 1024] [--chars 1000] [--num 1] [--calls 10] [--out FILE]

The page holds ``--chars`` chars laid out as text lines (tests/char_heatmap_restate.py text_line_quads).  Prints one JSON
object: kernel time per launch of every kernel the step runs (the context's timing table), launches per run, the host time
of ``run`` (the stream drained at its one synchronisation and after it), the Context.sync calls per run, and the time of the
restatement, which runs one char after the other as the reference does.  The step's result must equal the restatement's."""
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
    ap.add_argument('--num', type=int, default=1)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'text_region_label_kernels.json'))
    args = ap.parse_args()

    from vkit_amd import _native as N
    from vkit_amd.element import Image, Mask, Polygon
    from vkit_amd.pipeline.text_detection import (PageTextRegionLabelStepInput, PageTextRegionStepOutput,
                                                  page_text_region_label_step_factory as F)
    import char_heatmap_restate as HR
    import text_region_label_restate as R
    ctx = N.default_ctx()
    shape = (args.size, args.size)
    quads = HR.text_line_quads(default_rng(0), shape, args.chars, height=(16, 28), step=(0.75, 1.05))
    active = np.ones(shape, np.uint8)
    polygons = [Polygon.from_smooth_xy(q) for q in quads]
    src = PageTextRegionStepOutput(page_image=Image(mat=ctx.to_device(np.zeros(shape + (3,), np.uint8))),
                                   page_active_mask=Mask(mat=ctx.to_device(active)), page_char_polygons=polygons,
                                   page_text_region_polygons=polygons,
                                   page_char_polygon_text_region_polygon_indices=list(range(len(polygons))),
                                   shape_before_rotate=shape, rotate_angle=0, debug=None)
    step = F.create({'num_deviate_char_regression_labels': args.num})
    step_input = PageTextRegionLabelStepInput(page_text_region_step_output=src)

    out = step.run(step_input, default_rng(1))
    want = R.run(quads, shape, active, default_rng(1), num=args.num)
    assert out.page_char_mask.mat.tobytes() == want['char_mask'].tobytes()
    assert out.page_char_height_score_map.mat.tobytes() == want['height'].tobytes()
    assert out.page_char_gaussian_score_map.mat.tobytes() == want['gaussian'].tobytes()
    assert out.page_char_bounding_box_mask.mat.tobytes() == want['box_mask'].tobytes()
    labels = [(lb.char_idx, int(lb.tag.value == 'deviate'), lb.label_point_smooth_y, lb.label_point_smooth_x,
               lb.downsampled_label_point_y, lb.downsampled_label_point_x) for lb in out.page_char_regression_labels]
    assert labels == want['labels']

    ctx.sync()
    syncs = []
    real_sync = N.Context.sync
    N.Context.sync = lambda self: syncs.append(1) or real_sync(self)
    try:
        ctx.set_timing(1)
        ctx.reset_timings()
        for k in range(args.calls):
            step.run(step_input, default_rng(k))
        ctx.sync()
        syncs_per_run = (len(syncs) - 1) / args.calls
    finally:
        N.Context.sync = real_sync
    timings = ctx.timings()
    ctx.set_timing(0)
    kernels = {name: {'us_per_launch': round(ms * 1e3 / n, 2), 'launches_per_run': n / args.calls}
               for name, (ms, n) in sorted(timings.items())}
    device_us = sum(ms for ms, n in timings.values()) * 1e3 / args.calls
    # the same runs without timing events, the stream drained after each
    ctx.sync()
    t0 = time.perf_counter()
    for k in range(args.calls):
        step.run(step_input, default_rng(k))
        ctx.sync()
    host_ms = (time.perf_counter() - t0) * 1e3 / args.calls

    t0 = time.perf_counter()
    R.run(quads, shape, active, default_rng(1), num=args.num)
    restate_ms = (time.perf_counter() - t0) * 1e3
    result = {
        'page': list(shape), 'chars': len(quads), 'num_deviate': args.num,
        'labels': len(labels), 'layout': 'text lines, advance 0.75 .. 1.05 of the char width',
        'kernels': kernels,
        'launches_per_run': sum(v['launches_per_run'] for v in kernels.values()),
        'kernel_us_per_run': round(device_us, 2),
        'host_ms_per_run': round(host_ms, 3),
        'syncs_per_run': syncs_per_run,
        'restatement_ms_per_page': round(restate_ms, 1),
        'vkx_version': N.lib().vkx_version(),
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
