#!/usr/bin/env python3
"""Times the image, barcode, frame and symbol layers of one page: the four steps against the same planes made item by item.

    python tools/page_layers.py [--size 1024] [--calls 200] [--repeats 3] [--out FILE]

The page (seeded) carries 12 symbols, 2 QR codes, 1 code-39, 6 frames and 3 images.  ``steps``: PageImageStep, PageBarcodeStep,
PageTextLineBoundingBoxStep and PageNonTextSymbolStep rendering their plans inside ``_native.resident(True)`` -- one
vkx_page_layers_dev call a step.  ``item_by_item``: the same planes from the calls the library had before the steps existed --
``Image.to_resized_image`` a symbol, then its alpha in host numpy as the reference writes it; ``ScoreMap.to_resized_score_map``
a barcode (upload, resize, download, ``np.clip`` on the host); ``ScoreMap.from_shape`` and ``Box.fill_score_map`` a frame -- with
the same plans, so the draws are the same.  The image step is the same code both ways (it adds no kernel) and is timed in both.
Both ways are compared bit for bit before anything is timed.  Host plans (the generator draws, the encoders' stand-ins) are made
once, outside the timed window.  Prints one JSON object: per way the kernel time per launch (the context's timing table),
launches, kernel microseconds and Context.sync calls per page, and the host time per page of ``--repeats`` alternating windows
of ``--calls`` pages each, every window ended by a synchronise."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402


def write_textures(folder, R):
    """12 symbol files (RGBA and grayscale, 24 .. 96 pixels a side) and 3 pictures"""
    from PIL import Image as PilImage
    rng = np.random.default_rng(3)
    symbols, pictures = os.path.join(folder, 'symbols'), os.path.join(folder, 'pictures')
    os.makedirs(symbols)
    os.makedirs(pictures)
    for k in range(12):
        h, w = int(rng.integers(24, 97)), int(rng.integers(24, 97))
        if k % 3 == 2:
            tex = R.blocky(rng, (h, w), 4, 0, 2) * np.uint8(255)
        else:
            tex = rng.integers(0, 256, size=(h, w, 4)).astype(np.uint8)
            tex[:, :, 3] = R.blocky(rng, (h, w), 6, 0, 256)
        PilImage.fromarray(tex).save(os.path.join(symbols, f's{k:02d}.png'))
    for k in range(3):
        PilImage.fromarray(rng.integers(0, 256, size=(400, 500, 3)).astype(np.uint8)).save(os.path.join(pictures, f'p{k}.png'))
    return symbols, pictures


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'page_layers_kernels.json'))
    args = ap.parse_args()

    from vkit_amd import _native as N
    from vkit_amd.element import Box, Image, ScoreMap
    from vkit_amd.pipeline import text_detection as T
    import page_layers_restate as R
    ctx = N.default_ctx()
    size = args.size
    rng = np.random.default_rng(11)

    def box_of(h, w):
        up, left = int(rng.integers(0, size - h + 1)), int(rng.integers(0, size - w + 1))
        return Box(up=up, down=up + h - 1, left=left, right=left + w - 1)

    with tempfile.TemporaryDirectory() as folder:
        symbols_folder, pictures_folder = write_textures(folder, R)
        layout = T.PageLayoutStepOutput(page_layout=T.PageLayout(
            height=size, width=size,
            layout_images=[T.LayoutImage(box=box_of(int(rng.integers(150, 300)), int(rng.integers(200, 360)))) for _ in range(3)],
            layout_barcode_qrs=[T.LayoutBarcodeQr(box=box_of(s, s)) for s in (128, 190)],
            layout_barcode_code39s=[T.LayoutBarcodeCode39(box=box_of(64, 300))],
            layout_non_text_symbols=[T.LayoutNonTextSymbol(box=box_of(int(rng.integers(30, 130)), int(rng.integers(30, 130))),
                                                           alpha=float(rng.uniform(0.5, 1.0))) for _ in range(12)]))
        lines = []
        for k in range(6):
            h, w = int(rng.integers(24, 48)), int(rng.integers(200, 500))
            b = box_of(h, w)
            lines.append(R.text_line_of((b.up, b.down, b.left, b.right), [h], (20 * k, 0, 0), Box))
        frame_input = T.PageTextLineBoundingBoxStepInput(page_text_line_step_output=T.PageTextLineStepOutput(
            page_text_line_collection=T.PageTextLineCollection(height=size, width=size, text_lines=lines, short_text_line_flags=[False] * 6),
            page_seal_impression_text_line_collection=T.PageSealImpressionTextLineCollection(height=size, width=size)))

        image_step = T.PageImageStep(T.PageImageStepConfig(image_configs=[{'type': 'selector', 'config': {'image_folders': [pictures_folder]}}]))
        barcode_step = T.PageBarcodeStep(T.PageBarcodeStepConfig(), func_encode_qr=R.qr_image, func_encode_code39=R.code39_image)
        frame_step = T.PageTextLineBoundingBoxStep(T.PageTextLineBoundingBoxStepConfig(prob_non_short_text_line=1.0))
        symbol_step = T.PageNonTextSymbolStep(T.PageNonTextSymbolStepConfig(symbol_image_folders=[symbols_folder]))
        symbol_step.selector.image_files.sort()

        barcode_plan = barcode_step.plan(T.PageBarcodeStepInput(page_layout_step_output=layout), np.random.default_rng(1))
        frame_plans = frame_step.plan(frame_input, np.random.default_rng(2))
        symbol_plans = symbol_step.plan(T.PageNonTextSymbolStepInput(page_layout_step_output=layout), np.random.default_rng(3))
        assert (len(barcode_plan.qrs), len(barcode_plan.code39s), len(frame_plans), len(symbol_plans)) == (2, 1, 6, 12)
        image_input = T.PageImageStepInput(page_layout_step_output=layout)

        def steps():
            images = image_step.run(image_input, np.random.default_rng(4))
            barcodes = barcode_step.render(barcode_plan)
            frames = frame_step.render(frame_plans)
            symbols = symbol_step.render(symbol_plans)
            planes = list(barcodes.barcode_qr_score_maps) + list(barcodes.barcode_code39_score_maps) + list(frames.score_maps)
            return images, [p.arr for p in planes] + [p.arr for p in symbols.images] + [p.arr for p in symbols.alphas]

        def item_by_item():
            images = image_step.run(image_input, np.random.default_rng(4))
            planes, symbol_images, symbol_alphas = [], [], []
            for _, plan in barcode_plan.qrs + barcode_plan.code39s:
                mat = np.where(plan.mask > 0, np.float32(plan.alpha), np.float32(0)).astype(np.float32)
                score_map = ScoreMap(mat=mat)
                if score_map.shape != (plan.height, plan.width):
                    score_map = score_map.to_resized_score_map(resized_height=plan.height, resized_width=plan.width)
                planes.append(score_map.arr)
            for plan in frame_plans:
                score_map = ScoreMap.from_shape((plan.box_height, plan.box_width), value=plan.alpha)
                t = plan.border_thickness
                Box(up=t, down=plan.box_height - t - 1, left=t, right=plan.box_width - t - 1).fill_score_map(score_map, 0.0)
                up, down, left, right = plan.trims
                planes.append(np.ascontiguousarray(score_map.mat[up:plan.box_height - down, left:plan.box_width - right]))
            for plan in symbol_plans:
                image = Image(mat=plan.texture).to_resized_image(resized_height=plan.box.height, resized_width=plan.box.width)
                mat = image.mat
                if plan.symbol_color is None:
                    with np.errstate(invalid='ignore', divide='ignore'):
                        np_alpha = (mat[:, :, 3]).astype(np.float32) / 255
                        np_alpha_max = np_alpha.max()
                        np_alpha *= plan.alpha
                        np_alpha /= np_alpha_max
                    symbol_images.append(np.ascontiguousarray(mat[:, :, :3]))
                else:
                    np_alpha = (mat > 0).astype(np.float32)
                    np_alpha *= plan.alpha
                    symbol_images.append(Image.from_shape(mat.shape, value=plan.symbol_color).mat)
                symbol_alphas.append(np_alpha)
            return images, planes + symbol_images + symbol_alphas

        syncs = []
        real_sync = N.Context.sync
        N.Context.sync = lambda s: syncs.append(1) or real_sync(s)

        def kernels_of(call, calls):
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
            kernels = {name: {'us_per_launch': round(ms * 1e3 / n, 2), 'launches_per_page': n / calls} for name, (ms, n) in sorted(timings.items())}
            return dict(kernels=kernels, launches_per_page=sum(n for _, n in timings.values()) / calls,
                        kernel_us_per_page=round(sum(ms for ms, _ in timings.values()) * 1e3 / calls, 2),
                        context_syncs_per_page=n_syncs / calls)

        def host_ms(call, calls):
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(calls):
                call()
            ctx.sync()
            return round((time.perf_counter() - t0) * 1e3 / calls, 3)

        with N.resident(True):
            _, got = steps()
            _, want = item_by_item()
            assert len(got) == len(want)
            for k, (a, b) in enumerate(zip(got, want)):
                assert R.same_bits(N.host_array(a), N.host_array(b)), f'plane {k}: the steps and the item-by-item composition differ'
            result = {'steps': kernels_of(steps, args.calls), 'item_by_item': kernels_of(item_by_item, args.calls)}
            windows = {'steps': [], 'item_by_item': []}
            for _ in range(args.repeats):              # alternating windows: the spread is in the lists
                windows['steps'].append(host_ms(steps, args.calls))
                windows['item_by_item'].append(host_ms(item_by_item, args.calls))
        N.Context.sync = real_sync
        for key in windows:
            result[key]['host_ms_per_page'] = windows[key]

    result.update({
        'page_shape': [size, size], 'symbols': 12, 'barcode_qrs': 2, 'barcode_code39s': 1, 'frames': 6, 'images': 3,
        'calls_per_window': args.calls,
        'note': 'both ways include PageImageStep (the same code: three selector runs, the bottom layer and its rotation); the plans '
                '(draws, encoder stand-ins) are made once outside the windows; steps: planes stay on the device; item_by_item: the '
                'planes of the calls that existed before the steps, host arrays as those calls return them',
        'vkx_version': N.lib().vkx_version(),
    })
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
