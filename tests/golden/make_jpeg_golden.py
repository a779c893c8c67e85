"""Writes tests/golden/jpeg_roundtrip.npz: JPEG round trips through Pillow's libjpeg-turbo, the library the reference's
cv2 wheels bundle (``cv.imdecode(cv.imencode('.jpeg', mat, [IMWRITE_JPEG_QUALITY, q]))``, photometric/effect.py:41-42).

Run from the repository root: ``python tests/golden/make_jpeg_golden.py``.  A 3-channel mat is BGR to cv2, so Pillow is fed
``mat[..., ::-1]`` and its output flipped back (tests/jpeg_restate.py: pillow_roundtrip).

Layout: ``names`` (N,) str, ``libjpeg_turbo`` () str; per case i ``in_<i>`` (H, W[, 3]) uint8, ``q_<i>`` (Q_i,) int32 its
qualities and ``out_<i>`` (Q_i, H, W[, 3]) uint8, the round trip at each of them."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from jpeg_restate import pillow_roundtrip  # noqa: E402

QUALITIES = (1, 2, 10, 24, 25, 49, 50, 51, 75, 95, 100)
# height, width mod 16 cover {0, 1, odd, 8 +- 1}
SHAPES = ((1, 1), (1, 300), (300, 1), (7, 5), (8, 8), (9, 9), (15, 17), (16, 16), (17, 33), (97, 141), (256, 256), (1031, 23))
CONTENTS = ('random', 'gradient', 'saturated', 'asymmetric')


def content(kind, shape, rng):
    h, w = shape[:2]
    yy, xx = np.indices((h, w))
    if kind == 'random':
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == 'gradient':
        g = (yy * 255 // max(h - 1, 1) + xx * 255 // max(w - 1, 1)) // 2
        if len(shape) == 3:
            g = np.stack([g, 255 - g, (yy + 2 * xx) * 255 // max(h + 2 * w - 3, 1)], axis=-1)
        return g.astype(np.uint8)
    if kind == 'saturated':
        # 0/255 checkerboards of several pitches and hard edges: the blocks the inverse DCT overshoots the most
        s = (((yy // 1 + xx // 1) % 2) ^ (xx >= w // 2) ^ ((yy // 3) % 2 & (xx < w // 3))) * 255
        if len(shape) == 3:
            s = np.stack([s, 255 - s, ((xx // 4 + yy // 4) % 2) * 255], axis=-1)
        return s.astype(np.uint8)
    assert kind == 'asymmetric' and len(shape) == 3
    # channel 2 (R to the codec) saturated red stripes, channel 0 (B) a dark ramp, channel 1 noise around 40
    ch0 = (xx * 60 // max(w - 1, 1)).astype(np.int64)
    ch1 = 40 + rng.integers(-20, 21, (h, w))
    ch2 = np.where((xx // 3) % 2, 250, 10)
    return np.clip(np.stack([ch0, ch1, ch2], axis=-1), 0, 255).astype(np.uint8)


# The file stays small: the shapes up to 9 x 9 take every quality with every content; the other shapes deal the qualities out
# over their cases (RGB and grayscale contents in turn), a third of them each from 1 x 300 to 17 x 33, each quality once at 97 x 141,
# so that every shape still meets every quality; the large shapes take one content and a few qualities each.
LARGE = {((256, 256), 3): ('saturated', (1, 50, 95)), ((256, 256), 1): ('saturated', (2, 25, 100)),
         ((1031, 23), 3): ('saturated', (10, 75)), ((1031, 23), 1): ('gradient', (24, 51))}


def cases():
    rng = np.random.default_rng(20260915)
    for shape in SHAPES:
        dealt = 0
        for cn in (3, 1):
            full = shape + (3,) if cn == 3 else shape
            if (shape, cn) in LARGE:
                kind, qualities = LARGE[(shape, cn)]
                yield f'{shape[0]}x{shape[1]}x{cn}_{kind}', content(kind, full, rng), qualities
                continue
            kinds = [k for k in CONTENTS if cn == 3 or k != 'asymmetric']
            if shape == (97, 141) and cn == 3:
                kinds.remove('random')      # random RGB (hardly compressible) is covered at every smaller shape
            for kind in kinds:
                if shape == (97, 141):
                    qualities = QUALITIES[dealt % 6::6]
                elif shape[0] * shape[1] > 81:
                    qualities = QUALITIES[dealt % 3::3]
                else:
                    qualities = QUALITIES
                dealt += 1
                yield f'{shape[0]}x{shape[1]}x{cn}_{kind}', content(kind, full, rng), qualities


def main(path=os.path.join(HERE, 'jpeg_roundtrip.npz')):
    from PIL import features
    arrays = {'libjpeg_turbo': np.array(str(features.version_feature('libjpeg_turbo')))}
    names = []
    for i, (name, mat, qualities) in enumerate(cases()):
        names.append(name)
        arrays[f'in_{i}'] = mat
        arrays[f'q_{i}'] = np.array(qualities, np.int32)
        arrays[f'out_{i}'] = np.stack([pillow_roundtrip(mat, q) for q in qualities])
    arrays['names'] = np.array(names)
    np.savez_compressed(path, **arrays)
    print(path, len(names), 'cases', os.path.getsize(path), 'bytes, libjpeg-turbo', arrays['libjpeg_turbo'])


if __name__ == '__main__':
    main()
