#!/usr/bin/env python3
"""Regenerates tests/golden/page_layers.npz and .json by running THE REFERENCE's own PageNonTextSymbolStep, PageBarcodeStep,
PageTextLineBoundingBoxStep and the two barcode engines (vkit/pipeline/text_detection/, vkit/engine/barcode/) on small synthetic
inputs.

    python tests/golden/make_page_layers_golden.py

The missing third-party modules are stubbed as make_golden.py stubs them (it is imported for that), and ``barcode`` /
``barcode.writer`` likewise.  Patches, and only these: cv.resize -> oracle.resize; ``Code39(...).render()`` and
``cv.QRCodeEncoder.create().encode`` return the synthetic module images of tests/page_layers_restate.py (the encoders are
third-party code, absent here); Image.from_file reads the in-memory symbol textures; cattrs.structure stands in as
``cls(**mapping)``.  Everything else -- every draw, the inversion, the code-39 trim and its asserts, the score map, the resize and
the clip, the alpha rescale, the colour modes, the frame's offsets, ring, trims and asserts -- is the reference's code running
for real.

Stored, data only (arrays and the JSON index in the .npz, a list of the cases in the .json): the textures; per symbol run the
file list, boxes, alphas, config, seed, per symbol the file drawn, image, alpha plane and colour, and the generator's state
after the run; per barcode run the engine, config, shape, seed, text, module mask (after inversion and trim), alpha, score map
and state; the barcode page; per frame the page, text line, config, seed, every sampled value, the plane and the state; per
seeded frame page its lines and all of that per framed line.
"""
import json
import os
import sys
from types import SimpleNamespace
from unittest.mock import MagicMock

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden  # noqa: E402,F401  (stubs cv2 & co., puts the reference and this repository on sys.path)

for _m in ('barcode', 'barcode.writer'):
    sys.modules.setdefault(_m, MagicMock(name=_m))

import numpy as np  # noqa: E402
from numpy.random import default_rng  # noqa: E402

import cv2 as cv_stub  # noqa: E402  (the MagicMock)
import oracle as O  # noqa: E402
import page_layers_restate as R  # noqa: E402
from vkit.utility import opt as ref_opt  # noqa: E402
from vkit.element import Box, Image  # noqa: E402
from vkit.engine.barcode import code39 as C39, qr as QR  # noqa: E402
from vkit.engine.barcode.type import BarcodeEngineRunConfig  # noqa: E402
from vkit.pipeline.text_detection import page_barcode as PB, page_non_text_symbol as PS, page_text_line_bounding_box as PF  # noqa: E402

OUT = os.path.join(HERE, 'page_layers')
EQUAL_WEIGHTS = dict(weight_color_grayscale=1.0, weight_color_red=1.0, weight_color_green=1.0, weight_color_blue=1.0)


def layout_of(**fields):
    return SimpleNamespace(page_layout=SimpleNamespace(**fields))


def box_of(up, left, h, w):
    return Box(up=up, down=up + h - 1, left=left, right=left + w - 1)


def main():
    textures = R.symbol_textures()
    cv_stub.resize = lambda mat, dsize, interpolation=None: O.resize(mat, (dsize[1], dsize[0]), interpolation)
    ref_opt._cattrs.structure = lambda mapping, cls: cls(**mapping)
    drawn = []

    def from_file(cls, path, disable_exif_orientation=False):
        drawn.append(str(path))
        return cls(mat=textures[os.path.splitext(os.path.basename(str(path)))[0]].copy())
    Image.from_file = classmethod(from_file)
    texts = []
    cv_stub.QRCodeEncoder.create = lambda: SimpleNamespace(encode=lambda text: texts.append(text) or R.qr_image(text))
    C39.Code39 = lambda code, writer: SimpleNamespace(render=lambda: texts.append(code) or R.code39_image(code))
    C39.NoTextImageWriter = lambda: None

    packed = {}

    def put(array):
        array = np.ascontiguousarray(array)
        flat = packed.setdefault(str(array.dtype), [])
        at = sum(a.size for a in flat)
        flat.append(array.reshape(-1))
        return [at, list(array.shape), str(array.dtype)]

    # ---- symbols
    def symbol_run(name, files, layout, overrides, seed):
        step = PS.PageNonTextSymbolStep(PS.PageNonTextSymbolStepConfig(symbol_image_folders=[], **overrides))
        step.symbol_image_selector_engine_executor.engine.image_files = [f + '.png' for f in files]
        symbols = [SimpleNamespace(box=box_of(up, left, h, w), alpha=alpha) for up, left, h, w, alpha in layout]
        del drawn[:]
        rng = default_rng(seed)
        out = step.run(PS.PageNonTextSymbolStepInput(page_layout_step_output=layout_of(layout_non_text_symbols=symbols)), rng)
        rows = []
        for path, image, alpha in zip(drawn, out.images, out.alphas):
            assert isinstance(alpha, np.ndarray) and alpha.dtype == np.float32
            gray = textures[os.path.splitext(os.path.basename(path))[0]].ndim == 2
            rows.append(dict(file=os.path.splitext(os.path.basename(path))[0], image=put(image.mat), alpha=put(alpha),
                             color=[int(v) for v in image.mat[0, 0]] if gray else None))
        return dict(name=name, files=list(files), layout=[list(v) for v in layout], overrides=overrides, seed=seed, symbols=rows,
                    rng_state=rng.bit_generator.state)

    symbol_runs = []
    for k, (tex, shape, alpha) in enumerate(R.RGBA_CASES):
        symbol_runs.append(symbol_run(f'{tex}->{shape[0]}x{shape[1]}', [tex], [(0, 0, shape[0], shape[1], alpha)], {}, k))
    for tex, shape, alpha in R.GRAY_CASES:
        for seed in range(6):
            symbol_runs.append(symbol_run(f'{tex}->{shape[0]}x{shape[1]}', [tex], [(0, 0, shape[0], shape[1], alpha)], EQUAL_WEIGHTS, seed))
    files = [f for f in R.FILES if f != 'rgb_3ch']
    for seed in range(R.SYMBOL_PAGES):
        symbol_runs.append(symbol_run(f'page{seed}', files, R.symbol_page_layout(seed), {}, seed))

    # ---- barcode engines and the barcode page
    engines = dict(qr=(QR.BarcodeQrEngine, QR.BarcodeQrEngineInitConfig), code39=(C39.BarcodeCode39Engine, C39.BarcodeCode39EngineInitConfig))

    # the module mask of a run: the synthetic image through the reference's own inversion and trim
    def module_mask(kind, text):
        if kind == 'qr':
            return QR.Mask(mat=R.qr_image(text)).to_inverted_mask().mat
        return C39.BarcodeCode39Engine.convert_barcode_pil_image_to_mask(R.code39_image(text)).mat

    barcode_runs = []
    for kind, overrides, shape, seed in R.BARCODE_CASES:
        engine_cls, config_cls = engines[kind]
        engine = engine_cls(config_cls(**overrides))
        rng = default_rng(seed)
        del texts[:]
        score_map = engine.run(BarcodeEngineRunConfig(height=shape[0], width=shape[1]), rng)
        mask = module_mask(kind, texts[0])
        ink = score_map.mat[score_map.mat > 0]
        # the alpha drawn: replay the draws on a generator of its own (the reference keeps it in the map only)
        replay = default_rng(seed)
        if kind == 'qr':
            length = replay.integers(engine.init_config.payload_text_length_min, engine.init_config.payload_text_length_max + 1)
            replay.choice(len(engine.ascii_letters), size=length, replace=True)
        else:
            for _ in texts[0]:
                replay.choice(engine.ascii_letters)
        alpha = float(replay.uniform(engine.init_config.alpha_min, engine.init_config.alpha_max))
        assert replay.bit_generator.state == rng.bit_generator.state
        assert mask.shape != tuple(shape) or (ink == np.float32(alpha)).all()
        barcode_runs.append(dict(kind=kind, overrides=overrides, shape=list(shape), seed=seed, text=texts[0], mask=put(mask.astype(np.uint8)),
                                 alpha=alpha, score_map=put(score_map.mat), rng_state=rng.bit_generator.state))

    page = R.BARCODE_PAGE
    step = PB.PageBarcodeStep(PB.PageBarcodeStepConfig())
    rng = default_rng(page['seed'])
    del texts[:]
    out = step.run(PB.PageBarcodeStepInput(page_layout_step_output=layout_of(
        height=page['shape'][0], width=page['shape'][1], layout_barcode_qrs=[SimpleNamespace(box=box_of(*b)) for b in page['qrs']],
        layout_barcode_code39s=[SimpleNamespace(box=box_of(*b)) for b in page['code39s']])), rng)
    barcode_page = dict(texts=list(texts), qrs=[put(s.mat) for s in out.barcode_qr_score_maps],
                        code39s=[put(s.mat) for s in out.barcode_code39_score_maps], rng_state=rng.bit_generator.state)

    # ---- frames
    def frame_row(step, height, width, text_line, rng):
        """one sample_text_line_bounding_box with every sampled value recorded"""
        state = rng.bit_generator.state
        replay = default_rng(0)
        replay.bit_generator.state = state
        ref = max(g.ref_char_height for g in text_line.char_glyphs)
        offsets = [step.sample_offset(ref, replay) for _ in range(4)]
        thickness = step.sample_border_thickness(ref, replay)
        alpha = float(replay.uniform(step.config.alpha_max, step.config.alpha_max))
        score_map, color = step.sample_text_line_bounding_box(height, width, text_line, rng)
        assert replay.bit_generator.state == rng.bit_generator.state
        box_h = text_line.box.height + offsets[0] + offsets[1]
        box_w = text_line.box.width + offsets[2] + offsets[3]
        trims = [max(0, offsets[0] - text_line.box.up), max(0, text_line.box.down + offsets[1] - height + 1),
                 max(0, offsets[2] - text_line.box.left), max(0, text_line.box.right + offsets[3] - width + 1)]
        assert score_map.shape == (box_h - trims[0] - trims[1], box_w - trims[2] - trims[3])
        box = score_map.box
        return dict(offsets=offsets, thickness=thickness, alpha=alpha, box_shape=[box_h, box_w], trims=trims,
                    page_box=[box.up, box.down, box.left, box.right], color=[int(v) for v in color], plane=put(score_map.mat))

    frames = []
    sides = ('up', 'down', 'left', 'right')
    for name, (height, width, line_box, ref_h, overrides, want) in R.FRAME_CASES.items():
        for seed in range(1000):
            step = PF.PageTextLineBoundingBoxStep(PF.PageTextLineBoundingBoxStepConfig(**overrides))
            rng = default_rng(seed)
            try:
                row = frame_row(step, height, width, R.text_line_of(line_box, [ref_h], (10, 20, 30), Box), rng)
            except AssertionError:
                continue                     # (the reference's own asserts: an interior of fewer than two rows or columns)
            if tuple(s for s, t in zip(sides, row['trims']) if t) == want:
                break
        else:
            raise RuntimeError(f'no seed for frame case {name}')
        frames.append(dict(name=name, page=[height, width], line_box=list(line_box), ref_heights=[ref_h], overrides=overrides, seed=seed,
                           rng_state=rng.bit_generator.state, **row))
    # a frame trimmed down to its empty interior: all zeros
    for seed in range(1000):
        step = PF.PageTextLineBoundingBoxStep(PF.PageTextLineBoundingBoxStepConfig())
        rng = default_rng(seed)
        try:
            row = frame_row(step, 60, 100, R.text_line_of((20, 39, 10, 89), [20], (10, 20, 30), Box), rng)
        except AssertionError:
            continue
        at, shape, dtype = row['plane']
        if not packed[dtype][-1].any():
            frames.append(dict(name='interior_only', page=[60, 100], line_box=[20, 39, 10, 89], ref_heights=[20], overrides={}, seed=seed,
                               rng_state=rng.bit_generator.state, **row))
            break
    else:
        raise RuntimeError('no all-zero frame')
    assert frames[-2]['thickness'] == 1

    frame_runs = []
    for seed in R.FRAME_RUN_SEEDS:
        lines = R.frame_run_lines(seed)
        step = PF.PageTextLineBoundingBoxStep(PF.PageTextLineBoundingBoxStepConfig(**R.FRAME_RUN_CONFIG))
        rows = []
        real_sample = step.sample_text_line_bounding_box
        step.sample_text_line_bounding_box = lambda height, width, text_line, rng: (
            rows.append(frame_row(SimpleNamespace(sample_offset=step.sample_offset, sample_border_thickness=step.sample_border_thickness,
                                                  config=step.config, sample_text_line_bounding_box=real_sample),
                                  height, width, text_line, rng)) or
            (SimpleNamespace(), rows[-1]['color']))
        rng = default_rng(seed)
        collection = SimpleNamespace(height=160, width=220, text_lines=[R.text_line_of(b, hs, c, Box) for b, hs, c, _ in lines],
                                     short_text_line_flags=[short for _, _, _, short in lines])
        out = step.run(PF.PageTextLineBoundingBoxStepInput(page_text_line_step_output=SimpleNamespace(page_text_line_collection=collection)), rng)
        assert len(out.score_maps) == len(rows)
        frame_runs.append(dict(seed=seed, frames=rows, rng_state=rng.bit_generator.state))

    index = dict(symbol_runs=symbol_runs, barcode_runs=barcode_runs, barcode_page=barcode_page, frames=frames, frame_runs=frame_runs)
    np.savez_compressed(OUT + '.npz', index=np.array(json.dumps(index)), **{k: np.concatenate(v) for k, v in packed.items()},
                        **{'tex_' + k: v for k, v in textures.items()})
    with open(OUT + '.json', 'w') as f:
        json.dump(dict(symbol_runs=[[r['name'], r['seed'], len(r['symbols'])] for r in symbol_runs],
                       barcode_runs=[[r['kind'], r['shape'][0], r['shape'][1], r['seed']] for r in barcode_runs],
                       frames=[[r['name'], r['seed']] + r['trims'] for r in frames],
                       frame_runs=[[r['seed'], len(r['frames'])] for r in frame_runs]), f, indent=None, separators=(',', ':'))
        f.write('\n')
    print(OUT, os.path.getsize(OUT + '.npz'), '+', os.path.getsize(OUT + '.json'), 'bytes;', len(symbol_runs), 'symbol runs,',
          len(barcode_runs), 'barcode runs,', len(frames), 'frames,', sum(len(r['frames']) for r in frame_runs), 'frames in seeded pages')


if __name__ == '__main__':
    main()
