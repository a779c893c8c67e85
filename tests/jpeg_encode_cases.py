"""The cases of tests/golden/jpeg_encode.npz (tests/golden/make_jpeg_encode_golden.py), loaded once for the tests that share them."""
import functools
import os

import numpy as np


@functools.lru_cache(maxsize=None)
def _load(golden_dir):
    z = np.load(os.path.join(golden_dir, 'jpeg_encode.npz'))
    cases = []
    for i, name in enumerate(z['names']):
        mat = z[f'in_{i}']
        mat.flags.writeable = False
        for j, q in enumerate(z[f'q_{i}']):
            cases.append((str(name), mat, int(q), z[f'out_{i}_{j}'].tobytes()))
    return tuple(cases)


def golden_cases(golden_dir):
    """``(name, mat, quality, the file Pillow wrote)`` of every case; ``mat`` is uint8 H x W or H x W x 3 with channel 0 red."""
    return _load(golden_dir)
