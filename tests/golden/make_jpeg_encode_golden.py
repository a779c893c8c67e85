"""Writes tests/golden/jpeg_encode.npz: the JPEG files Pillow's libjpeg-turbo writes with its defaults
(``Image.save(f, format='JPEG', quality=q)``; reference image.py:351-359 saves through it), which the device encoder
(csrc/jpeg_encode.hip) and its restatement (tests/jpeg_encode_restate.py) reproduce to the byte.

Run from the repository root: ``python tests/golden/make_jpeg_encode_golden.py``.  Channel 0 is red (Pillow's mode RGB).

Layout: ``names`` (N,) str, ``pillow`` and ``libjpeg_turbo`` () str; per case i ``in_<i>`` (H, W[, 3]) uint8, ``q_<i>`` (Q_i,) int32
its qualities and ``out_<i>_<j>`` (bytes,) uint8 the file at quality ``q_<i>[j]``.

The maker asserts that the cases reach every event of the block coder (jpeg_encode_restate.REQUIRED_EVENTS) and prints which of
the two chance events of the stream's end it met."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import jpeg_encode_restate as E  # noqa: E402
from make_jpeg_golden import content as roundtrip_content  # noqa: E402

QUALITIES = (1, 10, 50, 75, 95, 100)
# height, width mod 16 cover {0, 1, 8 +- 1, 15}; 256 x 256 makes 1536 blocks and 156 chunks of unstuffed stream: 12 and 2 rounds of
# the 128-entry scan the device runs over an image of up to 2048 blocks
SHAPES = ((1, 1), (1, 300), (300, 1), (7, 5), (8, 8), (9, 9), (15, 17), (16, 16), (17, 33), (97, 141), (256, 256))
CONTENTS = ('random', 'gradient', 'saturated', 'asymmetric', 'constant')


def content(kind, shape, rng):
    if kind == 'constant':
        return np.full(shape, 77 if len(shape) == 2 else (200, 30, 90), np.uint8)
    if kind == 'blocks8':
        # whole 8 x 8 blocks alternately black and white: at quality 100 the DC differences are +-2040, category 11
        yy, xx = np.indices(shape[:2])
        s = (((yy // 8 + xx // 8) % 2) * 255).astype(np.uint8)
        return s if len(shape) == 2 else np.stack([s, s, s], axis=-1)
    return roundtrip_content(kind, shape, rng)


# The file stays small: the shapes up to 9 x 9 take every quality with every content; from 1 x 300 to 17 x 33 a case takes a third of
# the qualities, at 97 x 141 one, dealt out in turn so that every shape still meets every quality; 256 x 256 takes one content per
# mode.  The block alternation goes in at quality 100 where there are blocks to alternate.
LARGE = {((256, 256), 3): ('saturated', (10, 75, 100)), ((256, 256), 1): ('gradient', (1, 50, 75, 95))}
BLOCKS8 = ((17, 33), (97, 141))


def cases():
    rng = np.random.default_rng(20261021)
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
            if shape in BLOCKS8:
                yield f'{shape[0]}x{shape[1]}x{cn}_blocks8', content('blocks8', full, rng), (100,)


def main(path=os.path.join(HERE, 'jpeg_encode.npz')):
    import PIL
    from PIL import features
    arrays = {'pillow': np.array(PIL.__version__), 'libjpeg_turbo': np.array(str(features.version_feature('libjpeg_turbo')))}
    names = []
    census = dict.fromkeys(E.EVENTS, 0)
    for i, (name, mat, qualities) in enumerate(cases()):
        names.append(name)
        arrays[f'in_{i}'] = mat
        arrays[f'q_{i}'] = np.array(qualities, np.int32)
        for j, q in enumerate(qualities):
            data = E.pillow_encode(mat, q)
            arrays[f'out_{i}_{j}'] = np.frombuffer(data, np.uint8)
            restated, events = E.encode(mat, q)
            assert restated == data, (name, q)
            for key, count in events.items():
                census[key] += count
    missing = [e for e in E.REQUIRED_EVENTS if not census[e]]
    assert not missing, f'the cases never meet {missing}: add a case'
    arrays['names'] = np.array(names)
    np.savez_compressed(path, **arrays)
    print(path, len(names), 'cases', os.path.getsize(path), 'bytes, Pillow', arrays['pillow'], 'libjpeg-turbo', arrays['libjpeg_turbo'])
    print('census', census)
    print('chance events met:', [e for e in E.EVENTS[-2:] if census[e]] or 'neither')


if __name__ == '__main__':
    main()
