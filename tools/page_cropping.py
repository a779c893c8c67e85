#!/usr/bin/env python3
"""Times PageCroppingStep.run on a device-resident resized page against the reference-style host path on the same page.

    python tools/page_cropping.py [--size 2048] [--core 512] [--pad 64] [--samples 8] [--calls 20] [--out FILE]

Device leg: the seven planes live in HBM, run() issues k_crop_count + k_crop_planes and one download of the counts.
Host leg: the reference's loop in numpy on the same planes (tests/crop_restate.py: crop, count, INTER_AREA shrink), what
a caller without this step does after downloading the planes (download time included).  Prints one JSON object: kernel
time per launch (the context's timing table), launches and synchronisations per call, host time per call of each leg."""
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


def page_planes(size, seed=0):
    rng = default_rng(seed)
    active = np.zeros((size, size), np.uint8)
    active[size // 16:, : size - size // 16] = 1
    image = rng.integers(0, 256, (size, size, 3), dtype=np.uint8) * active[..., None]
    return dict(page_image=image, page_active_mask=active,
                page_char_mask=((rng.random((size, size)) < 0.1) * active).astype(np.uint8),
                page_seal_impression_char_mask=(rng.random((size, size)) < 0.01).astype(np.uint8),
                page_char_height_score_map=(rng.random((size, size), dtype=np.float32) * 8).astype(np.float32),
                page_text_line_mask=(rng.random((size, size)) < 0.2).astype(np.uint8),
                page_text_line_height_score_map=(rng.random((size, size), dtype=np.float32) * 8).astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=2048)
    ap.add_argument('--core', type=int, default=512)
    ap.add_argument('--pad', type=int, default=64)
    ap.add_argument('--samples', type=int, default=8)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--out')
    args = ap.parse_args()

    import crop_restate as R
    from vkit_amd import _native as N
    from vkit_amd.element import Image, Mask, ScoreMap
    from vkit_amd.pipeline.text_detection import (PageCroppingStep, PageCroppingStepConfig, PageCroppingStepInput,
                                                  PageResizingStepOutput)
    ctx = N.default_ctx()
    planes = page_planes(args.size)
    dev = {n: ctx.to_device(p) for n, p in planes.items()}
    page = PageResizingStepOutput(page_image=Image(mat=dev['page_image']),
                                  **{n: (ScoreMap(mat=dev[n], is_prob=False) if planes[n].dtype == np.float32 else Mask(mat=dev[n]))
                                     for n in R.PLANES[1:]})
    config = PageCroppingStepConfig(core_size=args.core, pad_size=args.pad, num_samples=args.samples)
    step = PageCroppingStep(config)
    step_input = PageCroppingStepInput(page_resizing_step_output=page)

    # sync count: hipStreamSynchronize / downloads through the context are what DevArray.host() and ctx.sync() issue
    syncs = [0]
    real_download = N.Context.download

    def counting_download(self, dptr, array):
        syncs[0] += 1
        return real_download(self, dptr, array)

    for _ in range(3):
        step.run(step_input, default_rng(0))
    ctx.sync()
    N.Context.download = counting_download
    ctx.set_timing(1)
    ctx.reset_timings()
    t0 = time.perf_counter()
    accepted = 0
    for i in range(args.calls):
        out = step.run(step_input, default_rng(i))
        accepted += len(out.cropped_pages)
    ctx.sync()
    device_s = (time.perf_counter() - t0) / args.calls
    N.Context.download = real_download
    timings = ctx.timings()
    ctx.set_timing(0)
    # untimed pass: host time without the event pairs
    t0 = time.perf_counter()
    for i in range(args.calls):
        step.run(step_input, default_rng(i))
    ctx.sync()
    device_untimed_s = (time.perf_counter() - t0) / args.calls

    is_prob = {n: False for n in R.LABELS}
    t0 = time.perf_counter()
    host_calls = max(1, args.calls // 4)
    for i in range(host_calls):
        host = {n: N.host_array(d).copy() for n, d in dev.items()}
        for d in dev.values():
            d.invalidate_host()
        R.run(host, config, default_rng(i), is_prob)
    host_s = (time.perf_counter() - t0) / host_calls

    result = dict(
        page=[args.size, args.size], core=args.core, pad=args.pad, num_samples=args.samples, calls=args.calls,
        accepted_per_call=accepted / args.calls,
        kernels={name: dict(ms_per_call=ms / args.calls, launches_per_call=n / args.calls,
                            us_per_launch=1e3 * ms / max(n, 1)) for name, (ms, n) in timings.items()},
        downloads_per_call=syncs[0] / args.calls,
        device_run_ms_per_call_timed=1e3 * device_s, device_run_ms_per_call=1e3 * device_untimed_s,
        host_numpy_ms_per_call=1e3 * host_s)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
