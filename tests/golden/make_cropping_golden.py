#!/usr/bin/env python3
"""Regenerates tests/golden/page_cropping.npz by running THE REFERENCE's own PageCroppingStep.run (vkit/pipeline/text_detection/
page_cropping.py) on small synthetic pages, many seeds.

    python tests/golden/make_cropping_golden.py

The missing third-party modules are stubbed exactly as make_golden.py stubs them (it is imported for that).  ONLY
cv.resize is oracle-patched: the stub is replaced by oracle.resize(src, (h, w), interpolation), which the step calls with
INTER_AREA for its downsampled labels.  Everything else -- the crop geometry, the generator's draws, the padding, the
counts and the accept / reject loop -- is the reference's code running for real.

Stored per case, in one JSON ``index`` row: the config, the seed, every attempted window in order (original_box, target_box,
original_core_box), the generator's state after ``run``, and where the seven input planes and every output plane of every
accepted crop sit in a few flat arrays (one per plane kind and dtype).  Data only, never reference source text.
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
from vkit.element import Image, Mask, ScoreMap  # noqa: E402
from vkit.mechanism import cropper as ref_cropper  # noqa: E402
from vkit.pipeline.text_detection import page_cropping as PC  # noqa: E402
from vkit.pipeline.text_detection.page_resizing import PageResizingStepOutput  # noqa: E402

OUT = os.path.join(HERE, 'page_cropping.npz')
LABELS = ('page_char_mask', 'page_seal_impression_char_mask', 'page_char_height_score_map', 'page_text_line_mask',
          'page_text_line_height_score_map')
PLANES = ('page_image', 'page_active_mask') + LABELS


def blocky(rng, shape, block, low, high, dtype):
    """Random values constant over block x block tiles (compresses well, still exercises every box sum)."""
    h, w = shape
    coarse = rng.integers(low, high, (-(-h // block), -(-w // block)))
    return np.kron(coarse, np.ones((block, block), np.int64))[:h, :w].astype(dtype)


def boxes_mask(rng, shape, n, size):
    h, w = shape
    mask = np.zeros(shape, np.uint8)
    for _ in range(n):
        bh, bw = (int(rng.integers(1, size + 1)) for _ in range(2))
        y, x = int(rng.integers(0, max(1, h - bh + 1))), int(rng.integers(0, max(1, w - bw + 1)))
        mask[y:y + bh, x:x + bw] = 1
    return mask


def make_page(seed, shape, active_frac, char_boxes, prob_score):
    rng = default_rng(10_000 + seed)
    h, w = shape
    image = np.stack([blocky(rng, shape, 4, 0, 16, np.uint8) * np.uint8(17) for _ in range(3)], axis=2)
    active = np.zeros(shape, np.uint8)
    ah, aw = max(1, int(h * active_frac)), max(1, int(w * active_frac))
    ay, ax = int(rng.integers(0, h - ah + 1)), int(rng.integers(0, w - aw + 1))
    active[ay:ay + ah, ax:ax + aw] = 1
    image = image * active[..., None]          # the page outside its active region is black, as after distortion
    char = boxes_mask(rng, shape, char_boxes, 6) * active
    seal = boxes_mask(rng, shape, 3, 8)
    line = boxes_mask(rng, shape, 6, 12)
    if prob_score:
        char_height = blocky(rng, shape, 2, 0, 5, np.float32) / np.float32(4)     # in [0, 1]
    else:
        char_height = blocky(rng, shape, 2, 0, 8, np.float32) * np.float32(1.37)
    line_height = (blocky(rng, shape, 3, 0, 8, np.float32) * np.float32(2.3)) * line
    return dict(page_image=image, page_active_mask=active, page_char_mask=char, page_seal_impression_char_mask=seal,
                page_char_height_score_map=char_height, page_text_line_mask=line,
                page_text_line_height_score_map=line_height.astype(np.float32))


# (name, page shape, config overrides, active fraction, char boxes, probability score map); each run with several seeds
LOWER = dict(text_ratio_min=0.0, active_region_ratio_min=0.05)
CASES = [
    ('larger', (80, 100), dict(core_size=32, pad_size=8), 0.9, 60, False),
    ('short_axis', (30, 200), dict(core_size=32, pad_size=8, **LOWER), 0.9, 40, False),
    ('short_axis_default', (40, 300), dict(core_size=64, pad_size=16), 0.9, 40, False),
    ('both_axes', (20, 30), dict(core_size=32, pad_size=8, **LOWER), 1.0, 10, False),
    ('crop_sized', (48, 48), dict(core_size=32, pad_size=8), 1.0, 30, False),
    ('num_samples_set', (90, 90), dict(core_size=24, pad_size=4, num_samples=3), 0.9, 50, False),
    ('num_samples_clamped', (90, 80), dict(core_size=24, pad_size=4, num_samples_max=2), 0.9, 50, False),
    ('num_samples_set_clamped', (80, 80), dict(core_size=24, pad_size=4, num_samples=5, num_samples_max=3), 0.9, 50, False),
    ('text_rejects', (100, 100), dict(core_size=32, pad_size=8, text_ratio_min=0.2), 0.9, 15, False),
    ('active_rejects', (100, 100), dict(core_size=32, pad_size=8, active_region_ratio_min=0.7), 0.5, 60, False),
    ('no_drops', (70, 90), dict(core_size=32, pad_size=8, drop_cropped_page_with_small_text_ratio=False,
                                drop_cropped_page_with_small_active_region=False), 0.4, 5, False),
    ('no_downsample', (70, 70), dict(core_size=32, pad_size=8, enable_downsample_labeling=False), 0.9, 60, False),
    ('factor4', (80, 80), dict(core_size=32, pad_size=8, downsample_labeling_factor=4), 0.9, 60, False),
    ('pad_value', (60, 50), dict(core_size=32, pad_size=8, pad_value=77, **LOWER), 0.8, 30, False),
    ('is_prob', (70, 80), dict(core_size=32, pad_size=8), 0.9, 60, True),
]
SEEDS = (0, 1, 2)


def box4(b):
    return [int(b.up), int(b.down), int(b.left), int(b.right)]


def main():
    saved_resize = cv_stub.resize
    # the ONLY oracle patch: cv.resize(mat, (w, h), interpolation) -> the oracle's restatement (INTER_AREA here)
    cv_stub.resize = lambda mat, dsize, interpolation=None: O.resize(mat, (dsize[1], dsize[0]), interpolation)
    attempts = []
    saved_init = ref_cropper.Cropper.__init__

    def recording_init(self, cropper_state):
        saved_init(self, cropper_state)
        attempts.append(cropper_state)

    PC.Cropper.__init__ = recording_init
    packed, index = {}, []

    def put(key, array):
        """Append ``array`` to the flat array ``key``: -> [offset, shape, dtype] for the index."""
        array = np.ascontiguousarray(array)
        parts = packed.setdefault((key, array.dtype.str), [])
        offset = sum(a.size for a in parts)
        parts.append(array.reshape(-1))
        return [key + array.dtype.str, offset, list(array.shape)]

    try:
        k = 0
        for name, shape, overrides, active_frac, char_boxes, prob in CASES:
            for seed in SEEDS:
                planes = make_page(seed * 31 + k, shape, active_frac, char_boxes, prob)
                config = PC.PageCroppingStepConfig(**overrides)
                resized = PageResizingStepOutput(
                    page_image=Image(mat=planes['page_image']),
                    **{n: (ScoreMap(mat=planes[n], is_prob=prob and n == 'page_char_height_score_map')
                           if planes[n].dtype == np.float32 else Mask(mat=planes[n])) for n in PLANES[1:]})
                rng = default_rng(seed)
                del attempts[:]
                got = PC.PageCroppingStep(config).run(PC.PageCroppingStepInput(page_resizing_step_output=resized), rng)
                row = dict(case=name, seed=seed, is_prob=bool(prob), config=overrides, rng_state=rng.bit_generator.state,
                           inputs={n: put('in_' + n, planes[n]) for n in PLANES},
                           attempts=[box4(s.original_box) + box4(s.target_box) + box4(s.original_core_box) for s in attempts],
                           samples=[])
                for page in got.cropped_pages:
                    sample = dict(target_core_box=box4(page.target_core_box), planes={'page_image': put('out_page_image',
                                                                                                        page.page_image.mat)})
                    for n in LABELS:
                        element = getattr(page, n)
                        assert element.box == page.target_core_box
                        sample['planes'][n] = put('out_' + n, element.mat)
                    if page.downsampled_label is not None:
                        d = page.downsampled_label
                        sample['down_shape'] = [int(v) for v in d.shape]
                        sample['down_target_core_box'] = box4(d.target_core_box)
                        for n in LABELS:
                            sample['planes']['down_' + n] = put('down_' + n, getattr(d, n).mat)
                    row['samples'].append(sample)
                index.append(row)
                k += 1
    finally:
        cv_stub.resize = saved_resize
        PC.Cropper.__init__ = saved_init
    # a handful of flat arrays and one JSON index: an npz member per plane would cost more in zip headers than in data
    out = {key + dtype: np.concatenate(parts) for (key, dtype), parts in packed.items()}
    out['index'] = np.array(json.dumps(index))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes')
    for k, row in enumerate(index):
        print(k, row['case'], row['seed'], 'samples', len(row['samples']), 'attempts', len(row['attempts']))


if __name__ == '__main__':
    main()
