"""Pins the JPEG encoder against a live Pillow -- only where one is installed (the goldens of tests/golden/jpeg_encode.npz hold
what Pillow 12.2.0 / libjpeg-turbo 3.1.4.1 wrote and need none).  On the CPU: the restatement on fresh random shapes and
qualities.  On the GPU: the device's bytes against Pillow's, and Pillow's decode of the device's bytes against the pinned round
trip (_native.jpeg_roundtrip), which ties the lossless half to the lossy one."""
import io
import os
import sys

import numpy as np
import pytest

PIL = pytest.importorskip('PIL')
from PIL import Image as PILImage, features  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import jpeg_encode_restate as E  # noqa: E402

VERSIONS = f'Pillow {PIL.__version__} / libjpeg-turbo {features.version_feature("libjpeg_turbo")} (pinned: 12.2.0 / 3.1.4.1)'


def fresh_cases(seed, count, side):
    rng = np.random.default_rng(seed)
    for i in range(count):
        h, w = (int(v) for v in rng.integers(1, side if i % 8 else 3 * side, 2))
        q = int(rng.integers(0, 101))
        shape = (h, w) if rng.random() < 0.3 else (h, w, 3)
        kind = i % 3
        if kind == 0:
            mat = rng.integers(0, 256, shape, dtype=np.uint8)
        elif kind == 1:
            mat = (rng.integers(0, 2, shape) * 255).astype(np.uint8)
        else:
            base = rng.integers(0, 256, ((h + 7) // 8, (w + 7) // 8) + shape[2:])      # flat 8 x 8 patches with a little noise
            mat = np.clip(np.repeat(np.repeat(base, 8, 0), 8, 1)[:h, :w] + rng.integers(-10, 11, shape), 0, 255).astype(np.uint8)
        yield i, mat, q


def compare(ours, pillow, what):
    """whole files; a header that differs over an equal scan is the Pillow version's, not the coder's"""
    if ours == pillow:
        return
    ours_header, ours_scan, _ = E.split_header(ours)
    pillow_header, pillow_scan, _ = E.split_header(pillow)
    if ours_scan == pillow_scan and ours_header != pillow_header:
        pytest.fail(f'{what}: the scans agree and the headers differ: a Pillow version difference, {VERSIONS}')
    pytest.fail(f'{what}: the scans differ ({len(ours_scan)} and {len(pillow_scan)} bytes), {VERSIONS}')


def test_restatement_equals_a_live_pillow_on_fresh_cases():
    for i, mat, q in fresh_cases(11, 120, 90):
        compare(E.encode_bytes(mat, q), E.pillow_encode(mat, q), (i, mat.shape, q))


@pytest.mark.gpu
def test_device_equals_a_live_pillow_on_fresh_cases():
    from vkit_amd import _native as N
    cases = list(fresh_cases(12, 96, 120))
    for quality in sorted({q for _i, _m, q in cases}):
        batch = [(i, mat) for i, mat, q in cases if q == quality]
        for (i, mat), ours in zip(batch, N.jpeg_encode([mat for _i, mat in batch], quality=quality)):
            compare(ours, E.pillow_encode(mat, quality), (i, mat.shape, quality))


@pytest.mark.gpu
def test_pillow_decodes_the_device_bytes_to_the_pinned_round_trip():
    from vkit_amd import _native as N
    for i, mat, q in fresh_cases(13, 24, 100):
        data = N.jpeg_encode([mat], quality=q)[0]
        decoded = np.asarray(PILImage.open(io.BytesIO(data)))
        if mat.ndim == 2:
            want = N.jpeg_roundtrip(mat, q)
        else:           # the round trip reads a mat as BGR
            want = N.jpeg_roundtrip(np.ascontiguousarray(mat[..., ::-1]), q)[..., ::-1]
        assert decoded.shape == mat.shape and (decoded == want).all(), (i, mat.shape, q)
