#!/usr/bin/env python3
"""Times the text-line labels of one page: PageTextLineLabelStep against the same labels composed quad by quad.

    python tools/text_line_label.py [--size 1024] [--lines 64] [--calls 20] [--out FILE]

The page's four planes come from ONE PageTextLineLabelStep.run, device-resident: vkx_box_label_masks_dev and
vkx_quad_interp_fill_dev.  The baseline composes the boundary score map as the reference's loop does, one
ScoreMap.fill_by_quad_interpolation(quad_v, keep_min_value=True) a quad on a device-resident map, then zeroes it outside the
boundary mask.  The step's planes are compared bit for bit with the numpy restatement (tests/text_line_label_restate.py) and with
the baseline before anything is timed.  Prints one JSON object: kernel time per launch (the context's timing table), launches
and Context.sync calls per page for both ways, and host time per page."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402


def page_lines(R, size, n_lines, seed=7):
    """``n_lines`` lines on a grid of cells, three in four horizontal, none in row 0"""
    rng = np.random.default_rng(seed)
    cols = max(1, int(np.sqrt(n_lines / 4)))
    rows = -(-n_lines // cols)
    cell_h, cell_w = size // rows, size // cols
    lines = []
    for k in range(n_lines):
        top, left = (k // cols) * cell_h, (k % cols) * cell_w
        if k % 4 == 3:      # vertical
            bh, bw = int(cell_h * 0.8), max(2, min(cell_w // 8, 24))
        else:
            bh, bw = max(2, min(int(cell_h * 0.5), 40)), int(cell_w * 0.85)
        up, lf = top + 1 + int(rng.integers(0, max(1, cell_h - bh - 1))), left + int(rng.integers(0, max(1, cell_w - bw)))
        font = min(bh, bw)
        lines.append(R.make_line((up, up + bh - 1, lf, lf + bw - 1), k % 4 != 3, font, sizes=(font,) * 12))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--lines', type=int, default=64)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'text_line_label_kernels.json'))
    args = ap.parse_args()

    from vkit_amd import _native as N
    from vkit_amd import element as E
    from vkit_amd.engine.font import type as FT
    from vkit_amd.pipeline import text_detection as T
    import text_line_label_restate as R
    ctx = N.default_ctx()
    shape = (args.size, args.size)
    lines = page_lines(R, args.size, args.lines)
    text_lines = [R.build_text_line(line, E, FT, reference=False) for line in lines]
    step_input = T.PageTextLineLabelStepInput(page_text_line_step_output=T.PageTextLineStepOutput(
        page_text_line_collection=T.PageTextLineCollection(height=shape[0], width=shape[1], text_lines=text_lines,
                                                           short_text_line_flags=[False] * len(lines)),
        page_seal_impression_text_line_collection=T.PageSealImpressionTextLineCollection(height=shape[0], width=shape[1])))
    step = T.page_text_line_label_step_factory.create(dict(enable_text_line_mask=True, enable_boundary_mask=True,
                                                           enable_boundary_score_map=True))
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

    boxes, dilated = step.generate_text_line_boxes_and_dilated_boxes(step_input.page_text_line_step_output.page_text_line_collection)
    quads = step.generate_boundary_quads(boxes, dilated)

    def quad_by_quad(boundary_mask):
        score_map = E.ScoreMap.from_unchecked_mat(ctx.to_device(np.ones(shape, np.float32)))
        for quad in quads:
            score_map.fill_by_quad_interpolation(*quad, func_np_uv_to_mat=E.quad_v, keep_min_value=True)
        boundary_mask.to_inverted_mask().fill_score_map(score_map, 0.0)
        return score_map

    with N.resident(True):
        out = step.run(step_input, None)
        want = R.step_planes(lines, shape, (True, True, True))
        got = dict(text_line_mask=out.page_text_line_mask, boundary_mask=out.page_text_line_boundary_mask,
                   text_line_and_boundary_mask=out.page_text_line_and_boundary_mask,
                   boundary_score_map=out.page_text_line_boundary_score_map)
        for key, plane in got.items():
            assert R.same_values(plane.mat, want[key]), f'{key}: the step and the restatement differ'
        assert R.same_values(quad_by_quad(out.page_text_line_boundary_mask).mat, want['boundary_score_map']), \
            'the quad-by-quad composition and the restatement differ'
        batched = measure(lambda: step.run(step_input, None), args.calls)
        baseline = measure(lambda: quad_by_quad(out.page_text_line_boundary_mask), max(1, args.calls // 4))

    result = {
        'page_shape': list(shape), 'text_lines': len(lines), 'quads': len(quads),
        'boundary_pixels': int(want['boundary_mask'].sum()),
        'step': batched, 'quad_by_quad_score_map_only': baseline,
        'note': 'step: all four planes and the host half (collections, tables); quad_by_quad: the boundary score map alone, one '
                'fill_by_quad_interpolation a quad on a device-resident map plus the zeroing fill; it also uploads the map of ones',
        'vkx_version': N.lib().vkx_version(),
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
