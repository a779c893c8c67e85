#!/usr/bin/env python3
"""Times the text lines of one synthetic page: the batched device call against the same lines composed from the per-call
operations.

    python tools/text_line.py [--lines 64] [--height 32] [--chars 24] [--calls 20] [--out FILE]

The page's lines are planned once (TextLineBatch.add is host work either way) and rendered by ONE vkx_text_lines_dev call,
device-resident.  The baseline walks every line as the reference does with the operations a caller had before the batched call
existed: Mask.fill_np_array and Box.fill_score_map(keep_max_value=True) per char, Image.to_resized_image,
Mask.to_resized_mask and ScoreMap.to_resized_score_map per resized line, the pad in numpy, and the glyph-mask and score-map fills
of the clean-up.  Both results are compared bit for bit before anything is timed.  A quarter of the lines is resized and a
quarter trimmed.  Prints one JSON object: kernel time per launch (the context's timing table), launches and Context.sync calls
per page for both ways, and host time per page."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402


def composed_baseline(plan):
    """the pixels of one planned line from the single-plane operations: (image, mask, score map | None) as numpy arrays"""
    from vkit_amd.element import Image, Mask, ScoreMap
    run_config, style = plan.run_config, plan.run_config.style
    height, width = plan.pasted
    np_image = np.full((height, width, 3), 255, np.uint8)
    np_mask = np.zeros((height, width), np.uint8)
    lcd = plan.char_glyphs[0].image.mat.ndim == 3
    score_map = None if lcd else ScoreMap.from_shape((height, width))
    for char_glyph, char_box in zip(plan.char_glyphs, plan.pasted_char_boxes):
        glyph_mask = char_glyph.get_glyph_mask(box=char_box.box)
        if lcd:
            value = ((1 - np.power(char_glyph.image.mat / 255.0, style.glyph_color_gamma)) * 255).astype(np.uint8)
        else:
            value = np.empty(char_glyph.image.shape + (3,), np.uint8)
            value[:] = style.glyph_color
        glyph_mask.fill_np_array(np_image, value)
        glyph_mask.fill_np_array(np_mask, 1)
        if score_map is not None:
            char_box.box.fill_score_map(score_map, char_glyph.score_map, keep_max_value=True)
    image, mask = Image(mat=np_image), Mask(mat=np_mask)
    interp = plan.cv_resize_interpolation
    if plan.resized != plan.pasted:
        size = dict(resized_height=run_config.height) if plan.is_hori else dict(resized_width=run_config.width)
        image = image.to_resized_image(cv_resize_interpolation=interp, **size)
        mask = mask.to_resized_mask(cv_resize_interpolation=interp, **size)
        if score_map is not None:
            score_map = score_map.to_resized_score_map(cv_resize_interpolation=interp, **size)
    full = (run_config.height, max(plan.resized[1], plan.out[1])) if plan.is_hori else (max(plan.resized[0], plan.out[0]), run_config.width)
    if full != plan.resized:
        rows, cols = slice(plan.pad_up, plan.pad_up + plan.resized[0]), slice(plan.pad_left, plan.pad_left + plan.resized[1])
        np_image = np.full(full + (3,), 255, np.uint8)
        np_image[rows, cols] = image.mat
        np_mask = np.zeros(full, np.uint8)
        np_mask[rows, cols] = mask.mat
        image, mask = Image(mat=np_image), Mask(mat=np_mask)
        if score_map is not None:
            np_score = np.zeros(full, np.float32)
            np_score[rows, cols] = score_map.mat
            score_map = ScoreMap(mat=np_score)
    if plan.cleanup:
        trimmed_idx, trimmed_box, kept_idx, kept_box = plan.cleanup
        glyph_mask = plan.char_glyphs[trimmed_idx].get_glyph_mask(box=trimmed_box, enable_resize=True, cv_resize_interpolation=interp)
        glyph_mask.fill_image(image, (255, 255, 255))
        glyph_mask.fill_mask(mask, 0)
        if score_map is not None:
            kept = plan.char_glyphs[kept_idx].score_map
            if kept.shape != kept_box.shape:
                kept = kept.to_resized_score_map(resized_height=kept_box.height, resized_width=kept_box.width, cv_resize_interpolation=interp)
            trimmed_box.fill_score_map(score_map, 0)
            kept_box.fill_score_map(score_map, kept, keep_max_value=True)
    out_h, out_w = plan.out
    return (np.ascontiguousarray(image.mat[:out_h, :out_w]), np.ascontiguousarray(mask.mat[:out_h, :out_w]),
            None if score_map is None else np.ascontiguousarray(score_map.mat[:out_h, :out_w]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lines', type=int, default=64)
    ap.add_argument('--height', type=int, default=32)
    ap.add_argument('--chars', type=int, default=24)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'text_line_kernels.json'))
    args = ap.parse_args()

    from vkit_amd import _native as N
    from vkit_amd.engine.font import plan_text_line, render_text_line_plans
    import text_line_restate as R
    ctx = N.default_ctx()
    rng = np.random.default_rng(7)
    letters = [c for c in R.CHARS if c not in '.HLT']
    plans = []
    for k in range(args.lines):
        text = ''.join(letters[int(i)] for i in rng.integers(0, len(letters), args.chars))
        resized, trimmed = k % 4 == 1, k % 4 == 2
        size = (args.height * 5) // 8 if resized else args.height - 4
        case = R._case(text, args.height, args.height * 6 if trimmed else 4000, size, seed=1000 + k,
                       enlarge=('CUBIC', 'LANCZOS4', 'LINEAR_EXACT')[k % 3])
        run_config, font_face, func, enlarge, shrink = R.amd_arguments(case)
        plan = plan_text_line(run_config, font_face, func, np.random.default_rng(case['seed']), enlarge, shrink)
        assert plan is not None
        plans.append(plan)
    n_resized = sum(plan.resized != plan.pasted for plan in plans)
    n_trimmed = sum(len(plan.char_boxes) < len(plan.char_glyphs) for plan in plans)
    n_cleanup = sum(plan.cleanup is not None for plan in plans)

    syncs = []
    real_sync = N.Context.sync
    N.Context.sync = lambda s: syncs.append(1) or real_sync(s)

    def measure(call, calls):
        call()
        ctx.sync()
        ctx.set_timing(1)
        ctx.reset_timings()
        del syncs[:]
        for _ in range(calls):
            call()
        n_syncs = len(syncs)
        ctx.sync()
        timings = ctx.timings()
        ctx.set_timing(0)
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        ctx.sync()
        host_ms = (time.perf_counter() - t0) * 1e3 / calls
        kernels = {name: {'us_per_launch': round(ms * 1e3 / n, 2), 'launches_per_page': n / calls} for name, (ms, n) in sorted(timings.items())}
        return dict(kernels=kernels, launches_per_page=sum(n for _, n in timings.values()) / calls,
                    kernel_us_per_page=round(sum(ms for ms, _ in timings.values()) * 1e3 / calls, 2),
                    context_syncs_per_page=n_syncs / calls, host_ms_per_page=round(host_ms, 3))

    with N.resident(True):
        lines = render_text_line_plans(plans)
        batched = measure(lambda: render_text_line_plans(plans), args.calls)
    for plan, line in zip(plans, lines):
        image, mask, score = composed_baseline(plan)
        assert R.same_bits(line.image.mat, image) and R.same_bits(line.mask.mat, mask), 'the batched call and the composition differ'
        assert (score is None) == (line.score_map is None) and (score is None or R.same_bits(line.score_map.mat, score))
    baseline = measure(lambda: [composed_baseline(plan) for plan in plans], max(1, args.calls // 10))

    result = {
        'lines': args.lines, 'line_height': args.height, 'chars_per_line': args.chars, 'lines_resized': n_resized,
        'lines_trimmed': n_trimmed, 'lines_cleaned_up': n_cleanup, 'output_pixels': int(sum(p.out[0] * p.out[1] for p in plans)),
        'batched': batched, 'composed_baseline': baseline,
        'note': 'planning (host) is outside both timings; context_syncs counts Context.sync calls; the baseline works on host arrays, '
                'so each of its operations also uploads and downloads its planes (synchronous copies)',
        'vkx_version': N.lib().vkx_version(),
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
