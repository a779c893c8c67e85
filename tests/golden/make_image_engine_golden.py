#!/usr/bin/env python3
"""Regenerates tests/golden/image_engine.npz by running THE REFERENCE's own ImageCombinerEngine.run, ImageSelectorEngine.run and
PageBackgroundStep.run (vkit/engine/image/, vkit/pipeline/text_detection/page_background.py) on a small in-memory texture set.

    python tests/golden/make_image_engine_golden.py

The missing third-party modules are stubbed exactly as make_golden.py stubs them (it is imported for that).  Oracle patches,
and only these: cv.GaussianBlur -> oracle.gaussian_blur, cv.warpAffine -> oracle.warp_affine, cv.resize -> oracle.resize;
Image.from_file and load_image_metas_from_folder read the in-memory texture set (iolite is absent).  cattrs is absent too: its
``structure(mapping, cls)`` stands in as ``cls(**mapping)``, the fallback the reference's dyn_structure has itself.  Everything
else -- the anchor sampling, the segment walk, the rotate-flag draws and the cache, the edge bands, the window and resize
choice, the aggregator's draw -- is the reference's code running for real.  The tile rectangles are recorded by wrapping
fill_np_edge_mask, which receives each tile's up, down, left, right.

Stored: the textures (one flat array) and their metas, and per case, in one JSON ``index`` row: the engine, the config
overrides, the run shape, the seed, the files the engine had cached when the run started, the tile list, the initial segments
of the run (the generator's draws replayed), the generator's state after the run and where the output sits in the flat output
array.  Data only, never reference source text.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402,F401  (stubs cv2 & co., puts the reference and this repository on sys.path)

import numpy as np  # noqa: E402
from numpy.random import default_rng  # noqa: E402

import cv2 as cv_stub  # noqa: E402  (the MagicMock)
import oracle as O  # noqa: E402
from vkit.utility import opt as ref_opt  # noqa: E402
from vkit.element import Image, ImageMode  # noqa: E402
from vkit.engine.image import combiner as RC, selector as RS  # noqa: E402
from vkit.engine.image.type import ImageEngineRunConfig  # noqa: E402
from vkit.pipeline.text_detection import page_background as PB  # noqa: E402
from vkit.pipeline.text_detection.page_shape import PageShapeStepOutput  # noqa: E402

OUT = os.path.join(HERE, 'image_engine.npz')

# (height, width, block, grayscale mean, grayscale std): sides 7 .. 90; 4 and 5 share their mean (the bisect ties)
TEXTURES = [
    (7, 9, 2, 80.0, 6.0), (12, 40, 3, 96.0, 5.0), (33, 21, 4, 101.0, 3.0), (90, 64, 8, 104.0, 4.0),
    (25, 25, 5, 110.0, 2.0), (18, 52, 6, 110.0, 7.0), (64, 90, 8, 118.0, 5.0), (45, 30, 5, 125.0, 9.0),
    (10, 11, 2, 131.0, 2.5), (72, 17, 4, 140.0, 6.0), (28, 77, 7, 150.0, 12.0), (50, 50, 10, 171.0, 4.0),
]


def texture_name(k):
    return f'{k:02d}.png'


def make_textures():
    rng = default_rng(20240607)
    out = []
    for h, w, block, mean, _ in TEXTURES:
        planes = []
        for _c in range(3):
            coarse = rng.integers(0, 8, (-(-h // block), -(-w // block)))
            planes.append(np.kron(coarse, np.ones((block, block), np.int64))[:h, :w])
        out.append(np.clip(np.stack(planes, axis=2) * 9 + int(mean) - 32, 0, 255).astype(np.uint8))
    return out


ALL = list(range(len(TEXTURES)))
# combiner: (name, init overrides, texture subset, (height, width), seeds, ksize or None, runs on one engine)
COMBINER = [
    ('anchor_only', dict(prob_use_only_the_anchor_image=1.0), ALL, (70, 100), (0, 1, 2), None, 1),
    ('several_metas', dict(prob_use_only_the_anchor_image=0.0), ALL, (96, 130), (0, 1, 2, 3), None, 1),
    ('rotate_never', dict(prob_use_only_the_anchor_image=0.0, prob_rotate_image=0.0), ALL, (80, 90), (0, 1), None, 1),
    ('rotate_always', dict(prob_use_only_the_anchor_image=0.0, prob_rotate_image=1.0), ALL, (80, 90), (0, 1), None, 1),
    ('rotate_half', dict(prob_use_only_the_anchor_image=0.0, prob_rotate_image=0.5), ALL, (90, 80), (0, 1, 2), None, 1),
    ('cache_off', dict(prob_use_only_the_anchor_image=0.0, enable_cache=False), ALL, (64, 64), (5,), None, 3),
    ('cache_on', dict(prob_use_only_the_anchor_image=0.0, enable_cache=True), ALL, (64, 64), (5, 6), None, 3),
    ('wider_than_segment', dict(prob_use_only_the_anchor_image=1.0, prob_rotate_image=0.0), [6], (100, 40), (0, 1), None, 1),
    ('taller_than_page', dict(prob_use_only_the_anchor_image=1.0, prob_rotate_image=0.0), [3, 9], (30, 120), (0, 1), None, 1),
    ('smaller_than_both', dict(prob_use_only_the_anchor_image=1.0), [0, 8], (40, 50), (0, 1), None, 1),
    ('narrow_page', dict(prob_use_only_the_anchor_image=0.0), ALL, (50, 3), (0, 1), None, 1),
    ('width_2', dict(prob_use_only_the_anchor_image=0.0), ALL, (20, 2), (0, 1, 2), None, 1),
    ('width_3', dict(prob_use_only_the_anchor_image=0.0, init_segment_width_min_ratio=0.5), ALL, (9, 3), (0, 1), None, 1),
    ('tall_page', dict(prob_use_only_the_anchor_image=0.0), ALL, (150, 37), (0, 1), None, 1),
    ('wide_page', dict(prob_use_only_the_anchor_image=0.0), ALL, (37, 150), (0, 1), None, 1),
    ('merge', dict(prob_use_only_the_anchor_image=1.0, prob_rotate_image=0.0), [6], (100, 60), (0, 1, 2), None, 1),
    ('ksize_3', dict(prob_use_only_the_anchor_image=0.0), ALL, (60, 70), (0, 1), 3, 1),
    ('ksize_7', dict(prob_use_only_the_anchor_image=0.0), ALL, (60, 70), (0, 1), 7, 1),
    ('height_1', dict(prob_use_only_the_anchor_image=0.0), ALL, (1, 40), (0,), None, 1),
]
# selector: (name, init overrides, texture subset, run config, seeds)
SELECTOR = [
    ('window', dict(), [3, 6, 11], dict(height=20, width=30), (0, 1, 2)),
    ('window_whole', dict(), [11], dict(height=50, width=50), (0,)),
    ('too_small', dict(), [0, 8], dict(height=20, width=30), (0, 1)),
    ('force_resize', dict(force_resize=True), [3, 6, 11], dict(height=20, width=30), (0, 1)),
    ('disable_resizing', dict(), ALL, dict(height=0, width=0, disable_resizing=True), (0, 1)),
    ('mode_none', dict(target_image_mode=None), [3, 6, 11], dict(height=33, width=17), (0, 1)),
]
# background: (name, step overrides, engines [(type, weight, overrides, subset)], (height, width), seeds)
BACKGROUND = [
    ('key_image', dict(weight_image=1.0, weight_random_grayscale=0.0),
     [('combiner', 1, dict(prob_use_only_the_anchor_image=0.0), ALL)], (60, 80), (0, 1)),
    ('key_grayscale', dict(weight_image=0.0, weight_random_grayscale=1.0, grayscale_min=100, grayscale_max=200),
     [('combiner', 1, dict(), ALL)], (40, 30), (0, 1)),
    ('both_keys', dict(), [('combiner', 1, dict(), ALL)], (48, 56), (0, 1, 2, 3, 4, 5)),
    ('two_engines', dict(weight_image=1.0, weight_random_grayscale=0.0),
     [('combiner', 3, dict(prob_use_only_the_anchor_image=0.0), ALL), ('selector', 1, dict(), [3, 6, 11])], (30, 40),
     (0, 1, 2, 3, 4, 5, 6, 7)),
]


def replay_initial_segments(rng, n_metas, init_config, width):
    """The initial segments of a combiner run whose generator is ``rng`` (a copy, taken before the run)."""
    rng.choice(n_metas)
    rng.random()
    segment_width_min = int(np.clip(round(init_config.init_segment_width_min_ratio * width), 1, width - 1))
    segments, left = [], 0
    while left + segment_width_min - 1 < width:
        right = int(rng.integers(left + segment_width_min - 1, width))
        if right + 1 - left < segment_width_min or width - right - 1 < segment_width_min:
            break
        segments.append([left, right])
        left = right + 1
    if left < width:
        segments.append([left, width - 1])
    return segments


def copy_rng(rng):
    other = default_rng(0)
    other.bit_generator.state = rng.bit_generator.state
    return other


def main():
    textures = make_textures()
    by_name = {texture_name(k): t for k, t in enumerate(textures)}
    subset = {'now': ALL}

    saved = (cv_stub.GaussianBlur, cv_stub.warpAffine, cv_stub.resize, ref_opt._cattrs.structure, Image.__dict__['from_file'],
             RC.load_image_metas_from_folder, RC.ImageCombinerEngine.__dict__['fill_np_edge_mask'])
    cv_stub.GaussianBlur = lambda mat, ksize, sigma: O.gaussian_blur(mat, ksize[0], sigma)
    cv_stub.warpAffine = lambda mat, trans_mat, dsize: O.warp_affine(mat, trans_mat, dsize)
    cv_stub.resize = lambda mat, dsize, interpolation=None: O.resize(mat, (dsize[1], dsize[0]), interpolation)
    ref_opt._cattrs.structure = lambda mapping, cls: cls(**mapping)
    Image.from_file = classmethod(lambda cls, path, disable_exif_orientation=False: cls(mat=by_name[os.path.basename(str(path))].copy()))
    RC.load_image_metas_from_folder = lambda folder: [
        RC.ImageMeta(image_file='image/' + texture_name(k), grayscale_mean=TEXTURES[k][3], grayscale_std=TEXTURES[k][4])
        for k in subset['now']]
    tiles = []
    edge_fill = saved[6].__func__

    def recording_fill(cls, **kw):
        tiles.append([int(kw[n]) for n in ('up', 'down', 'left', 'right')])
        return edge_fill(cls, **kw)

    RC.ImageCombinerEngine.fill_np_edge_mask = classmethod(recording_fill)

    index, outputs = [], []

    def put(array):
        array = np.ascontiguousarray(array)
        assert array.dtype == np.uint8
        offset = sum(a.size for a in outputs)
        outputs.append(array.reshape(-1))
        return [offset, list(array.shape)]

    def jsonable(overrides):
        return {k: (v.value if isinstance(v, ImageMode) else v) for k, v in overrides.items()}

    try:
        for name, overrides, metas, shape, seeds, ksize, runs in COMBINER:
            for seed in seeds:
                subset['now'] = metas
                config_cls = RC.ImageCombinerEngineInitConfig
                if ksize is not None:
                    config_cls = type('Ksize%dInitConfig' % ksize, (config_cls,), dict(gaussian_blur_kernel_size=ksize))
                init_config = config_cls(image_meta_folder='unused', **overrides)
                engine = RC.ImageCombinerEngine(init_config)
                rng = default_rng(seed)
                for run in range(runs):
                    del tiles[:]
                    cached = sorted(os.path.basename(f) for f in engine.image_file_to_cache_image)
                    segments = replay_initial_segments(copy_rng(rng), len(metas), init_config, shape[1])
                    got = engine.run(ImageEngineRunConfig(height=shape[0], width=shape[1]), rng)
                    assert got.mat.shape == shape + (3,) and got.mode == ImageMode.RGB
                    index.append(dict(kind='combiner', case=name, seed=seed, run=run, overrides=jsonable(overrides), metas=metas,
                                      shape=list(shape), ksize=ksize, cached_before=cached, tiles=[list(t) for t in tiles],
                                      init_segments=segments, rng_state=rng.bit_generator.state, out=put(got.mat),
                                      mode=got.mode.value))
        for name, overrides, files, run_config, seeds in SELECTOR:
            for seed in seeds:
                engine = RS.ImageSelectorEngine(RS.ImageSelectorEngineInitConfig(image_folders=['unused'], **overrides))
                engine.image_files = ['image/' + texture_name(k) for k in files]
                rng = default_rng(seed)
                got = engine.run(ImageEngineRunConfig(**run_config), rng)
                index.append(dict(kind='selector', case=name, seed=seed, overrides=jsonable(overrides), files=files,
                                  run_config=run_config, rng_state=rng.bit_generator.state, out=put(got.mat), mode=got.mode.value))
        for name, overrides, engines, shape, seeds in BACKGROUND:
            for seed in seeds:
                image_configs = []
                for type_name, weight, engine_overrides, _ in engines:
                    config = dict(engine_overrides)
                    config.update(dict(image_meta_folder='unused') if type_name == 'combiner' else dict(image_folders=['unused']))
                    image_configs.append(dict(type=type_name, weight=weight, config=config))
                subset['now'] = [e[3] for e in engines if e[0] == 'combiner'][0]
                step = PB.PageBackgroundStep(PB.PageBackgroundStepConfig(image_configs=image_configs, **overrides))
                for executor, (type_name, _, _, files) in zip(step.image_engine_executor_aggregator.selector.engine_executors, engines):
                    if type_name == 'selector':
                        executor.engine.image_files = ['image/' + texture_name(k) for k in files]
                rng = default_rng(seed)
                del tiles[:]
                got = step.run(PB.PageBackgroundStepInput(PageShapeStepOutput(height=shape[0], width=shape[1])), rng).background_image
                assert got.mat.shape == tuple(shape) + (3,)
                index.append(dict(kind='background', case=name, seed=seed, overrides=overrides,
                                  engines=[[t, w, jsonable(o), f] for t, w, o, f in engines], shape=list(shape),
                                  tiles=[list(t) for t in tiles], rng_state=rng.bit_generator.state, out=put(got.mat),
                                  mode=got.mode.value))
    finally:
        cv_stub.GaussianBlur, cv_stub.warpAffine, cv_stub.resize, ref_opt._cattrs.structure = saved[:4]
        Image.from_file = saved[4]
        RC.load_image_metas_from_folder = saved[5]
        RC.ImageCombinerEngine.fill_np_edge_mask = saved[6]

    offsets = np.cumsum([0] + [t.size for t in textures])
    np.savez_compressed(
        OUT, textures=np.concatenate([t.reshape(-1) for t in textures]), texture_offsets=offsets,
        texture_shapes=np.array([t.shape for t in textures]), metas=np.array([[m, s] for _, _, _, m, s in TEXTURES]),
        outputs=np.concatenate(outputs), index=np.array(json.dumps(index)))
    print(OUT, os.path.getsize(OUT), 'bytes', len(index), 'cases')
    for k, row in enumerate(index):
        print(k, row['kind'], row['case'], row['seed'], row.get('run', ''), len(row.get('tiles', ())), 'tiles')


if __name__ == '__main__':
    main()
