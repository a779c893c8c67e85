#!/usr/bin/env python3
"""Times the text-line score maps of one page's seal impressions: the batched device call against the same work composed per
char from the single-plane operations.

    python tools/seal_fill.py [--seals 2] [--size 256] [--chars 40] [--calls 20] [--out FILE]

The page's seals go through ONE fill_text_lines_to_seal_impressions call (vkx_seal_fill_dev), device-resident.  The baseline
walks the chars as the reference does and uses the operations a caller had before the batched call existed:
ScoreMap.to_resized_score_map, rotate.distort and Box.fill_score_map(keep_max_value=True) per char, then the maximum and the
rescale in numpy.  Both results are compared bit for bit before anything is timed.  Prints one JSON object: kernel time per
launch (the context's timing table), launches and Context.sync calls per page for both ways, and host time per page."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402


def per_char_baseline(item):
    """fill_text_line_to_seal_impression of one seal composed per char from the single-plane operations (score-map glyphs)"""
    import attrs
    from vkit_amd.element import Box, Point, ScoreMap
    from vkit_amd.mechanism.distortion import rotate
    seal_impression, indices, text_lines, internal = item
    assert internal is None
    score_map = ScoreMap.from_shape(seal_impression.shape)
    for slot_index, text_line in zip(indices, text_lines):
        slot = seal_impression.text_line_slots[slot_index]
        ref = max(text_line.char_glyphs, key=lambda g: g.ref_char_height)
        factor = slot.char_aspect_ratio / (ref.ref_char_width / ref.ref_char_height)
        for char_box, glyph, char_slot in zip(text_line.char_boxes, text_line.char_glyphs, slot.char_slots):
            resized_width = max(1, round(factor * glyph.width))
            resized_box = attrs.evolve(char_box.box, left=0, right=resized_width - 1)
            plane = ScoreMap.from_shape((text_line.box.height, resized_width))
            glyph_map = glyph.score_map
            if glyph_map.shape != resized_box.shape:
                glyph_map = glyph_map.to_resized_score_map(resized_height=resized_box.height, resized_width=resized_box.width,
                                                           cv_resize_interpolation=text_line.cv_resize_interpolation)
            resized_box.fill_score_map(plane, glyph_map)
            rotated = rotate.distort({'angle': char_slot.angle - 270}, score_map=plane, point=Point.create(y=0, x=resized_width / 2),
                                     disable_clip_result_elements=True)
            up = char_slot.point_up.y - rotated.point.y
            left = char_slot.point_up.x - rotated.point.x
            down, right = up + rotated.score_map.height - 1, left + rotated.score_map.width - 1
            if up < 0 or down >= score_map.height or left < 0 or right >= score_map.width:
                continue
            Box(up=up, down=down, left=left, right=right).fill_score_map(score_map, rotated.score_map, keep_max_value=True)
    with np.errstate(invalid='ignore', divide='ignore'):
        return score_map.mat * seal_impression.alpha / score_map.mat.max()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seals', type=int, default=2)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--chars', type=int, default=40)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'seal_fill_kernels.json'))
    args = ap.parse_args()

    from vkit_amd import _native as N
    from vkit_amd.engine.seal_impression import fill_text_lines_to_seal_impressions
    import seal_impression_restate as R
    ctx = N.default_ctx()
    cases = [R.make_case(seed=100 + k, shape=(args.size, args.size), n_chars=(args.chars,), heights=(24,), interp='CUBIC',
                         widths=(8, 20), reach=0.8) for k in range(args.seals)]
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
        device_items = [R.amd_items(case, device=True) for case in cases]
        results = fill_text_lines_to_seal_impressions(device_items)
        batched = measure(lambda: fill_text_lines_to_seal_impressions(device_items), args.calls)
    host_items = [R.amd_items(case) for case in cases]
    placed = [len(polygons) for _, polygons in results]
    for item, (score_map, _) in zip(host_items, results):
        assert R.same_bits(score_map.mat, per_char_baseline(item)), 'the batched call and the per-char composition differ'
    baseline = measure(lambda: [per_char_baseline(item) for item in host_items], max(1, args.calls // 4))

    result = {
        'seals': args.seals, 'seal_shape': [args.size, args.size], 'chars_per_seal': args.chars, 'chars_placed': placed,
        'batched': batched, 'per_char_baseline': baseline,
        'note': 'context_syncs counts Context.sync calls; the baseline also downloads every resized and rotated plane (synchronous copies)',
        'vkx_version': N.lib().vkx_version(),
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
