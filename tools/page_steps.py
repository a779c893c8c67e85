#!/usr/bin/env python3
"""Wall time of the three pipeline callers of the path on a C4-shaped synthetic page (1024^2, 64 text lines, 384 char
polygons): PageAssemblerStep.run, PageDistortionStep.run, PageResizingStep.run -- host arrays in, host arrays out -- and
where the host time goes (cProfile, top cumulative entries).  Usage: tools/page_steps.py [size] [n_lines] > out.json

    tools/page_steps.py text_region_cropping [size] [out.json]

runs one leg alone: PageTextRegionCroppingStep.run on a device-resident page (default 1024^2) whose label counts are those of
the largest case of tests/golden/text_region_cropping.npz times the ratio of the page sides; the record (default
profiles/text_region_cropping_kernels.json) holds the kernel time of k_region_crop_select and of k_crop_planes, the step's wall
time, the wall time of the selection call alone and, beside them, the wall time of the numpy restatement of the selection
(tests/text_region_cropping_restate.py) on the same tables and windows.

    tools/page_steps.py text_region_flatten [size] [out.json]

runs the pixel half of PageTextRegionStep on a device-resident synthetic page (default 1024^2, 128 text-line-shaped regions) two
ways: the batched path of csrc/region_flatten.hip (build_flattened_text_regions, resize_flattened_text_regions,
post_rotate_flattened_text_regions, stack_flattened_text_regions) and the same work composed per region from the single-plane
operators (Mask.extract_image, rotate.distort, the external box in numpy, to_cropped_image, to_resized_image / to_resized_mask,
Box.fill_image / fill_mask).  The record (default profiles/text_region_flatten_kernels.json) holds, for each, the wall time, the
time of every kernel and the dispatch counts per page.

    tools/page_steps.py contours [size] [out.json]

runs Mask.to_disconnected_polygons (csrc/contours.hip) on a device-resident page mask (default 1024^2) of 64 slanted text-line
quads, and masks_to_disconnected_polygons on a batch of 128 device-resident pair masks of about 40 x 300.  The record (default
profiles/contours_kernels.json) holds, for each, the time of every kernel, the dispatch count and the wall time of a call."""
import cProfile
import io
import json
import os
import pstats
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import attrs
import numpy as np
from numpy.random import default_rng

from vkit_amd.pipeline.text_detection.synthetic_page import synthetic_page_input as _synthetic_page_input
from vkit_amd import _native as N
from vkit_amd.pipeline import text_detection as T

LEG = len(sys.argv) > 1 and sys.argv[1] in ('text_region_cropping', 'text_region_flatten', 'contours')
size = int(sys.argv[1]) if len(sys.argv) > 1 and not LEG else 1024
n_lines = int(sys.argv[2]) if len(sys.argv) > 2 and not LEG else 64
ctx = N.default_ctx()
step_input = _synthetic_page_input(seed=3, size=size, n_lines=n_lines)
assembler = T.page_assembler_step_factory.create()
distortion = T.page_distortion_step_factory.create()
resizing = T.page_resizing_step_factory.create()


PER_RUN = {}


def timed(fn, reps, label=None):
    fn(0)
    ctx.set_timing(True); ctx.reset_timings()
    each = []
    t0 = time.perf_counter()
    for k in range(reps):
        t1 = time.perf_counter()
        fn(k + 1)
        each.append(time.perf_counter() - t1)
    dt = (time.perf_counter() - t0) / reps
    kernels = {n: round(v[0] / reps, 4) for n, v in ctx.timings().items()}
    ctx.set_timing(False)
    if label:
        each.sort()
        PER_RUN[label] = {'median_ms': round(each[len(each) // 2] * 1e3, 3), 'min_ms': round(each[0] * 1e3, 3),
                          'max_ms': round(each[-1] * 1e3, 3), 'runs': reps}
    return dt, kernels


def top(fn, reps, n=14):
    pr = cProfile.Profile()
    pr.enable()
    for k in range(reps):
        fn(100 + k)
    pr.disable()
    res = {}
    for key in ('cumulative', 'tottime'):
        buf = io.StringIO()
        pstats.Stats(pr, stream=buf).sort_stats(key).print_stats(n)
        res[key] = [l.strip().replace(ROOT + '/', '') for l in buf.getvalue().splitlines() if l.strip() and l.strip()[0].isdigit()][:n + 1]
    return res


def text_region_cropping_leg(size, path):
    import text_region_cropping_restate as R
    from vkit_amd.element import Image, Mask, Point, ScoreMap
    from vkit_amd.pipeline.text_detection import page_text_region_cropping as M
    largest = max(R.load_golden(), key=lambda r: len(r['label_key']))
    scale = size // max(largest['shape'])
    n_chars = (int(largest['label_key'][:, 1].max()) + 1) * scale
    rng = default_rng(11)
    tags = (T.PageCharRegressionLabelTag.CENTROID, T.PageCharRegressionLabelTag.DEVIATE)
    labels = []
    for g in range(n_chars):
        cy, cx = rng.uniform(8, size - 8, 2).tolist()
        corners = [Point.create(y=cy + dy, x=cx + dx) for dy, dx in ((-6, -5), (-6, 5), (6, 5), (6, -5))]
        for tag in (0, 1):
            y, x = (cy, cx) if tag == 0 else (cy + rng.uniform(-4, 4), cx + rng.uniform(-3, 3))
            labels.append(T.PageCharRegressionLabel(char_idx=g, tag=tags[tag], label_point_smooth_y=y, label_point_smooth_x=x,
                                                    downsampled_label_point_y=round(y), downsampled_label_point_x=round(x),
                                                    up_left=corners[0], up_right=corners[1], down_right=corners[2],
                                                    down_left=corners[3]))
    shape = (size, size)
    planes = dict(page_image=rng.integers(0, 256, shape + (3,), dtype=np.uint8), char=rng.integers(0, 2, shape, dtype=np.uint8),
                  height=rng.random(shape, dtype=np.float32) * 30, gaussian=rng.random(shape, dtype=np.float32),
                  box=rng.integers(0, 2, shape, dtype=np.uint8))
    dev = {k: ctx.to_device(v) for k, v in planes.items()}
    config = dict(core_size=size * 3 // 8, pad_size=size // 16)
    pages = 4
    step = T.page_text_region_cropping_step_factory.create(config)
    step_in = T.PageTextRegionCroppingStepInput(
        page_cropping_step_output=T.PageCroppingStepOutput(cropped_pages=[None] * pages),
        page_text_region_step_output=T.PageTextRegionStepOutput(
            page_image=Image(mat=dev['page_image']), page_active_mask=Mask(mat=np.ones(shape, np.uint8)), page_char_polygons=[],
            page_text_region_polygons=[], page_char_polygon_text_region_polygon_indices=[], shape_before_rotate=shape,
            rotate_angle=0, debug=None),
        page_text_region_label_step_output=T.PageTextRegionLabelStepOutput(
            page_char_mask=Mask(mat=dev['char']), page_char_height_score_map=ScoreMap(mat=dev['height'], is_prob=False),
            page_char_gaussian_score_map=ScoreMap(mat=dev['gaussian']), page_char_regression_labels=labels,
            page_char_bounding_box_mask=Mask(mat=dev['box'])))
    reps = 20
    samples = len(step.run(step_in, default_rng(0)).cropped_page_text_regions)
    dt, kernels = timed(lambda s: step.run(step_in, default_rng(s)), reps, 'step')
    centroid = M.label_table([lb for lb in labels if lb.tag == tags[0]])
    deviate = M.label_table([lb for lb in labels if lb.tag == tags[1]])
    probe = default_rng(1)
    windows = M.core_box_table([step._state(shape, shape, 0, probe) for _ in range(max(3, 2 * pages))])

    def median_ms(fn):
        fn()
        each = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            each.append(time.perf_counter() - t0)
        return round(sorted(each)[reps // 2] * 1e3, 4)

    record = {
        'page': f'{size}x{size}', 'chars': n_chars, 'centroid_labels': len(centroid), 'deviate_labels': len(deviate),
        'candidate_windows': len(windows), 'samples': samples, 'config': config, 'runs': reps,
        'kernel_ms_per_run': kernels,
        'step_wall_ms': dict(PER_RUN['step'], mean_ms=round(dt * 1e3, 3)),
        'label_table_build_wall_ms': median_ms(lambda: (M.label_table(labels[0::2]), M.label_table(labels[1::2]))),
        'selection_call_wall_ms': median_ms(lambda: N.region_crop_select(windows, centroid, deviate, ctx=ctx)),
        'numpy_selection_wall_ms': median_ms(lambda: R.select(windows, centroid, deviate)),
        'note': 'selection_call_wall_ms is _native.region_crop_select alone (staging, launch, the three copies back, the '
                'synchronisation); numpy_selection_wall_ms the restatement R.select on the same tables and windows; both are part of, '
                'or stand for a part of, step_wall_ms, which also builds the label tables from the label objects '
                '(label_table_build_wall_ms), crops and shifts the kept labels',
    }
    with open(path, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')
    print(json.dumps(record, indent=1))


def text_region_flatten_leg(size, path):
    from vkit_amd.element import Box, Image, Mask
    from vkit_amd.mechanism.distortion import rotate
    from vkit_amd.pipeline.text_detection import page_text_region as F
    rng = default_rng(17)
    n_regions, reps = 128, 10
    page = rng.integers(0, 256, (size, size, 3), dtype=np.uint8)
    masks_host, angles, heights, post = [], [], [], []
    for _ in range(n_regions):
        bh, bw = int(rng.integers(16, 49)), int(rng.integers(60, min(400, size // 2) + 1))
        up, left = int(rng.integers(0, size - bh + 1)), int(rng.integers(0, size - bw + 1))
        mat = np.ones((bh, bw), np.uint8)
        mat[:2], mat[-2:], mat[:, :3] = 0, 0, 0                      # the band around a dilated text line
        masks_host.append((mat, Box(up=up, down=up + bh - 1, left=left, right=left + bw - 1)))
        angles.append(int(rng.choice([*range(350, 360), *range(1, 11)])))
        heights.append(int(rng.integers(32, 47)))                    # the sampled char height decides the resized height
        post.append(int(rng.choice([0, 0, 0, 0, 180, 180, 90, 270])))
    image = Image(mat=ctx.to_device(page))
    masks = [Mask(mat=ctx.to_device(mat), box=box) for mat, box in masks_host]

    def batched(_):
        regions = F.TextRegionFlattener.build_flattened_text_regions(image, [None] * n_regions, masks, (), angles, None)
        regions = F.resize_flattened_text_regions(regions, [(h, None) for h in heights])
        regions = F.post_rotate_flattened_text_regions(regions, post)
        out = F.stack_flattened_text_regions(0, 2, regions, F.ColumnPacker)
        ctx.sync()
        return out

    def per_region(_):
        regions = []
        for mask, angle, height, post_angle in zip(masks, angles, heights, post):
            result = rotate.distort({'angle': angle}, image=mask.extract_image(image), mask=mask)
            np_mask = result.mask.mat > 0
            rows, cols = np.nonzero(np_mask.any(axis=1))[0], np.nonzero(np_mask.any(axis=0))[0]
            box = Box(up=int(rows[0]), down=int(rows[-1]), left=int(cols[0]), right=int(cols[-1]))
            region_image = result.image.to_cropped_image(up=box.up, down=box.down, left=box.left, right=box.right)
            region_mask = box.extract_mask(result.mask)
            region_image = region_image.to_resized_image(resized_height=height)
            region_mask = region_mask.to_resized_mask(resized_height=height)
            if post_angle:
                result = rotate.distort({'angle': post_angle}, image=region_image, mask=region_mask)
                region_image, region_mask = result.image, result.mask
            regions.append((region_image, region_mask))
        width = max(r.width for r, _ in regions) + 4
        height = sum(r.height + 4 for r, _ in regions)
        stacked = Image(mat=ctx.to_device(F.build_background_image_for_stacking(height, width).mat))
        active = Mask(mat=N.dev_zeros((height, width), np.uint8, ctx=ctx))
        y = 0
        for region_image, region_mask in regions:
            box = Box(up=y + 2, down=y + 2 + region_image.height - 1, left=2, right=2 + region_image.width - 1)
            box.fill_image(stacked, region_image, image_mask=region_mask)
            box.fill_mask(active, 1, mask_mask=region_mask)
            y += region_image.height + 4
        ctx.sync()
        return stacked, active

    def measure(fn):
        fn(0)
        ctx.sync()
        ctx.set_timing(True)
        ctx.reset_timings()
        each = []
        for k in range(reps):
            t0 = time.perf_counter()
            fn(k + 1)
            each.append(time.perf_counter() - t0)
        timings = ctx.timings()
        ctx.set_timing(False)
        each.sort()
        return {'wall_ms': {'median_ms': round(each[reps // 2] * 1e3, 3), 'min_ms': round(each[0] * 1e3, 3),
                            'max_ms': round(each[-1] * 1e3, 3)},
                'kernel_ms_per_page': {name: round(ms / reps, 4) for name, (ms, _cnt) in sorted(timings.items())},
                'dispatches_per_page': {name: round(cnt / reps, 2) for name, (_ms, cnt) in sorted(timings.items())},
                'dispatches_per_page_total': round(sum(cnt for _ms, cnt in timings.values()) / reps, 2)}

    with N.resident(True):
        new_image, new_active = batched(0)[:2]
        old_image, old_active = per_region(0)
        agree = bool(np.array_equal(new_image.mat, old_image.mat) and np.array_equal(new_active.mat, old_active.mat))
        record = {'page': f'{size}x{size}', 'regions': n_regions, 'runs': reps, 'stacked_page': list(new_image.shape),
                  'paths_agree': agree, 'batched': measure(batched), 'per_region': measure(per_region),
                  'note': 'both paths start from a device-resident page and device-resident masks, leave the stacked page and its '
                          'active mask on the device and end with one Context.sync; wall_ms includes the host work of each path '
                          '(records and states for the batched one, per-region element objects, the download of every rotated mask '
                          'for its external box and the host crops for the other); kernel times are measured with event pairs, '
                          'which add a few microseconds a dispatch to the wall time of both'}
    with open(path, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')
    print(json.dumps(record, indent=1))


def contours_leg(size, path):
    from vkit_amd.element import Mask
    from vkit_amd.element.mask import masks_to_disconnected_polygons
    rng = default_rng(23)
    reps = 20
    yy, xx = np.mgrid[:size, :size]
    page = np.zeros((size, size), np.uint8)
    for k in range(64):                                               # 64 text lines, 7 px thick, slanted by 1 .. 2 px in 100
        slope, centre = rng.uniform(0.01, 0.02), (k + 0.5) * size / 64
        page |= ((np.abs(yy - (centre + slope * (xx - size / 2))) <= 3) & (xx >= size // 25) & (xx < size - size // 25)).astype(np.uint8)
    pairs = []
    for _ in range(128):                                              # a precise polygon cut by a text region: a slanted band
        h, w = int(rng.integers(30, 51)), int(rng.integers(250, 351))
        y, x = np.mgrid[:h, :w]
        slope = rng.uniform(-0.03, 0.03)
        pairs.append(((np.abs(y - (h / 2 + slope * (x - w / 2))) <= h / 4) & (x >= 3) & (x < w - 3)).astype(np.uint8))
    page_mask = Mask(mat=ctx.to_device(page))
    pair_masks = [Mask(mat=ctx.to_device(mat)) for mat in pairs]

    def measure(fn):
        out = fn()
        ctx.sync()
        calls = []
        real = N.mask_contours_raw
        N.mask_contours_raw = lambda *a, **k: calls.append(1) or real(*a, **k)
        ctx.set_timing(True)
        ctx.reset_timings()
        each = []
        try:
            for _ in range(reps):
                t0 = time.perf_counter()
                fn()
                each.append(time.perf_counter() - t0)
            timings = ctx.timings()
        finally:
            ctx.set_timing(False)
            N.mask_contours_raw = real
        each.sort()
        return {'polygons': sum(len(polygons) for polygons in out), 'points': sum(p.num_points for polygons in out for p in polygons),
                'contour_calls_per_call': round(len(calls) / reps, 2),
                'wall_ms': {'median_ms': round(each[reps // 2] * 1e3, 3), 'min_ms': round(each[0] * 1e3, 3), 'max_ms': round(each[-1] * 1e3, 3)},
                'kernel_ms_per_call': {name: round(ms / reps, 4) for name, (ms, _cnt) in sorted(timings.items())},
                'kernel_ms_per_call_total': round(sum(ms for ms, _cnt in timings.values()) / reps, 4),
                'dispatches_per_call': round(sum(cnt for _ms, cnt in timings.values()) / reps, 2)}

    record = {'runs': reps, 'method': 'CHAIN_APPROX_SIMPLE',
              'page_mask': dict(measure(lambda: [page_mask.to_disconnected_polygons()]), shape=[size, size], text_lines=64),
              'pair_masks': dict(measure(lambda: masks_to_disconnected_polygons(pair_masks)), masks=len(pair_masks),
                                 pixels=int(sum(mat.size for mat in pairs))),
              'note': 'device-resident masks; a call ends with its one copy-out and one Context.sync and wall_ms includes the host '
                      'work of the element layer (records, the polygons built from the points); kernel times are measured with event '
                      'pairs, which add a few microseconds a dispatch to the wall time; contour_calls_per_call is 2 where the default '
                      'capacities were short and the call was repeated with the sizes the first one reported'}
    with open(path, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')
    print(json.dumps(record, indent=1))


if LEG and sys.argv[1] == 'contours':
    contours_leg(int(sys.argv[2]) if len(sys.argv) > 2 else 1024,
                 sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, 'profiles', 'contours_kernels.json'))
    sys.exit(0)
if LEG and sys.argv[1] == 'text_region_flatten':
    text_region_flatten_leg(int(sys.argv[2]) if len(sys.argv) > 2 else 1024,
                            sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, 'profiles', 'text_region_flatten_kernels.json'))
    sys.exit(0)
if LEG:
    text_region_cropping_leg(int(sys.argv[2]) if len(sys.argv) > 2 else 1024,
                             sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, 'profiles', 'text_region_cropping_kernels.json'))
    sys.exit(0)


out = {'page': f'{size}x{size}', 'text_lines': n_lines}
page_out = assembler.run(step_input, default_rng(0))
dt, k = timed(lambda s: assembler.run(step_input, default_rng(s)), 10, 'page_assembler')
out['page_assembler'] = {'ms': round(dt * 1e3, 3), 'kernel_ms_per_run': k, 'gpu_ms': round(sum(k.values()), 3),
                         'profile_top': top(lambda s: assembler.run(step_input, default_rng(s)), 6)}
dt, k = timed(lambda s: assembler.run(step_input, default_rng(s)).page.image.mat, 10, 'page_assembler_outputs_on_host')
out['page_assembler_outputs_on_host'] = {'ms': round(dt * 1e3, 3), 'note': 'the same runs with the assembled page read on the host afterwards'}
dist_in = T.PageDistortionStepInput(page_out)
dist_out = distortion.run(dist_in, default_rng(0))
dt, k = timed(lambda s: distortion.run(dist_in, default_rng(s)), 48, 'page_distortion')
out['page_distortion'] = {'ms': round(dt * 1e3, 3), 'kernel_ms_per_run': k, 'gpu_ms': round(sum(k.values()), 3),
                          'profile_top': top(lambda s: distortion.run(dist_in, default_rng(s)), 6)}


def touch(step_output):
    """Reads every pixel element of a step output on the host (``.mat`` downloads a device-resident element)."""
    for field in attrs.fields(type(step_output)):
        value = getattr(step_output, field.name)
        if hasattr(value, 'mat'):
            value.mat
    return step_output


dt, k = timed(lambda s: touch(distortion.run(dist_in, default_rng(s))), 48, 'page_distortion_outputs_on_host')
out['page_distortion_outputs_on_host'] = {'ms': round(dt * 1e3, 3), 'note': 'the same runs with every output element read on the host afterwards'}
res_in = T.PageResizingStepInput(page_distortion_step_output=dist_out)
try:
    dt, k = timed(lambda s: resizing.run(res_in, default_rng(s)), 10, 'page_resizing')
    out['page_resizing'] = {'ms': round(dt * 1e3, 3), 'kernel_ms_per_run': k, 'gpu_ms': round(sum(k.values()), 3)}
    dt, k = timed(lambda s: touch(resizing.run(res_in, default_rng(s))), 10, 'page_resizing_outputs_on_host')
    out['page_resizing_outputs_on_host'] = {'ms': round(dt * 1e3, 3)}
    chain_in = lambda s: T.PageResizingStepInput(page_distortion_step_output=distortion.run(dist_in, default_rng(s)))
    dt, k = timed(lambda s: touch(resizing.run(chain_in(s), default_rng(s))), 48, 'distortion_then_resizing_outputs_on_host')
    out['distortion_then_resizing_outputs_on_host'] = {'ms': round(dt * 1e3, 3), 'gpu_ms': round(sum(k.values()), 3),
                                                       'note': 'PageDistortionStep.run -> PageResizingStep.run, resized outputs read on the host: the full-size label planes never cross the link'}
except Exception as exc:      # the step refuses pages without text lines of a minimum height
    out['page_resizing'] = {'error': repr(exc)}
for name, stats in PER_RUN.items():
    out[name]['per_run'] = stats
out['note'] = ('page_distortion: the mean over 48 seeds includes the pages whose RandomDistortion draws poisson_noise (one sequential '
               'numpy rng.poisson call, ~95 ms for a 1024^2 page, see DESIGN): the median is the typical page')
print(json.dumps(out, indent=1))
