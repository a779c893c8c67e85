#!/usr/bin/env python3
"""Times the combiner image engine on one GPU and writes profiles/image_engine_steps.json:

  kernel   k_image_combine for a 1024^2 and a 2048^2 page from 256^2 textures (median of warm runs, HIP events on the launch
           stream) beside a device-to-device copy of the same page in the same run, timed by the same events, and their ratio;
  engine   wall time of ImageCombinerEngine.run per page (warm cache, device-resident) beside the numpy restatement
           (tests/image_engine_restate.py) on one thread;
  page     PageBackgroundStep + PageAssemblerStep per page with the background resident, beside the assembler fed the same
           background as a host array.

    python tools/image_engine_steps.py [--runs 50] [--out profiles/image_engine_steps.json]
    python tools/image_engine_steps.py --launches 2048      # only a few warm launches at that page side: the command a counter
                                                            # run wraps (tools/pmc_any.sh image_combine k_image_combine python ...)

Run each GPU step of a longer job under its own time limit, e.g. ``timeout -k 10 300 python tools/image_engine_steps.py``."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
from numpy.random import default_rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def make_folder(folder, n=8, side=256):
    import image_engine_restate as R
    rng = default_rng(0)
    textures = [np.repeat(np.repeat(rng.integers(0, 256, (side // 8, side // 8, 3), dtype=np.uint8), 8, axis=0), 8, axis=1) for _ in range(n)]
    metas = [(100.0 + k, 10.0) for k in range(n)]
    return R.write_folder(folder, textures, metas), textures


def event_ms(ctx, name, fn, runs):
    """Median milliseconds of kernel ``name`` over ``runs`` calls of ``fn`` (one launch each)."""
    out = []
    ctx.set_timing(1)
    try:
        for _ in range(runs):
            ctx.reset_timings()
            fn()
            ms, cnt = ctx.timings()[name]
            assert cnt == 1
            out.append(ms)
    finally:
        ctx.set_timing(0)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=50)
    ap.add_argument('--launches', type=int, default=0, help='page side: run 10 warm launches and nothing else')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'image_engine_steps.json'))
    args = ap.parse_args()
    os.environ.setdefault('OMP_NUM_THREADS', '1')
    import image_engine_restate as R
    from vkit_amd import _native as N
    from vkit_amd.element import Image
    from vkit_amd.engine.image import ImageCombinerEngine, ImageCombinerEngineInitConfig, ImageEngineRunConfig
    from vkit_amd.pipeline import text_detection as T
    from vkit_amd.pipeline.text_detection.synthetic_page import synthetic_page_input

    ctx = N.default_ctx()
    result = dict(runs=args.runs, kernel={}, engine={}, page={})
    with tempfile.TemporaryDirectory() as tmp:
        folder, textures = make_folder(os.path.join(tmp, 'set'))
        config = ImageCombinerEngineInitConfig(image_meta_folder=folder, prob_use_only_the_anchor_image=0.0, sigma=30.0, enable_cache=True)
        engine = ImageCombinerEngine(config)
        if args.launches:
            with N.resident(True):
                for seed in range(10):
                    engine.run(ImageEngineRunConfig(height=args.launches, width=args.launches), default_rng(seed))
            ctx.sync()
            return
        for side in (1024, 2048):
            run_config = ImageEngineRunConfig(height=side, width=side)
            with N.resident(True):
                for seed in range(5):
                    page = engine.run(run_config, default_rng(seed))
                kernel = event_ms(ctx, 'k_image_combine', lambda: engine.run(run_config, default_rng(7)), args.runs)
                # the yardstick: a device-to-device copy of the same page on the same stream, on the same clock (the library
                # brackets a device copy with HIP events as it brackets a kernel: "copy_d2d")
                copy = event_ms(ctx, 'copy_d2d', lambda: N.device_copy(page.arr), args.runs)
                walls = []
                for k in range(args.runs):
                    ctx.sync()
                    t0 = time.perf_counter()
                    engine.run(run_config, default_rng(100 + k))
                    ctx.sync()
                    walls.append((time.perf_counter() - t0) * 1e3)
            result['kernel'][str(side)] = dict(k_image_combine_ms=kernel, copy_d2d_ms=copy, ratio=kernel / copy)
            restate = R.Combiner(config, engine.image_metas, {m.image_file: t for m, t in zip(
                sorted(engine.image_metas, key=lambda m: m.image_file), textures)})
            t0 = time.perf_counter()
            n = max(1, args.runs // 10)
            for k in range(n):
                restate.run(side, side, default_rng(100 + k))
            result['engine'][str(side)] = dict(engine_wall_ms=statistics.median(walls), restatement_wall_ms=(time.perf_counter() - t0) * 1e3 / n)

        # the page path: C4-shaped page, background resident against the same background as a host array
        size = 1024
        step = T.page_background_step_factory.create(dict(
            image_configs=[dict(type='combiner', config=dict(image_meta_folder=folder, enable_cache=True))], weight_image=1.0,
            weight_random_grayscale=0.0))
        assembler = T.page_assembler_step_factory.create()
        shape_input = T.PageBackgroundStepInput(T.PageShapeStepOutput(height=size, width=size))
        page_input = synthetic_page_input(seed=7, size=size, n_lines=64)
        host_background = Image(mat=np.array(step.run(shape_input, default_rng(0)).background_image.mat))
        for mode in ('host', 'resident'):
            times = []
            ctx.set_timing(1)
            ctx.reset_timings()
            for k in range(args.runs + 3):
                ctx.sync()
                t0 = time.perf_counter()
                with N.resident(mode == 'resident'):
                    if mode == 'resident':
                        background = step.run(shape_input, default_rng(k)).background_image
                    else:
                        background = host_background
                    page_input.page_background_step_output = T.PageBackgroundStepOutput(background)
                    assembler.run(page_input, default_rng(0))
                ctx.sync()
                if k >= 3:
                    times.append((time.perf_counter() - t0) * 1e3)
            timings = ctx.timings()
            ctx.set_timing(0)
            result['page'][mode] = dict(wall_ms=statistics.median(times),
                                        kernel_ms_per_page={name: ms / (args.runs + 3) for name, (ms, cnt) in timings.items() if cnt})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fout:
        json.dump(result, fout, indent=1)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
