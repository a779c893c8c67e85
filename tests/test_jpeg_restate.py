"""jpeg_quality's round trip (photometric/effect.py:41-42) on the CPU: tests/jpeg_restate.py against the libjpeg-turbo fixtures of
tests/golden/jpeg_roundtrip.npz and, where Pillow is installed, against the library itself; the C entry points of the device
kernel are declared and exported."""
import ctypes
import io
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import jpeg_restate as J  # noqa: E402


def golden_cases(golden_dir):
    z = np.load(os.path.join(golden_dir, 'jpeg_roundtrip.npz'))
    for i, name in enumerate(z['names']):
        yield str(name), z[f'in_{i}'], z[f'q_{i}'], z[f'out_{i}']


def test_restatement_equals_every_golden_case(golden_dir):
    z = np.load(os.path.join(golden_dir, 'jpeg_roundtrip.npz'))
    assert str(z['libjpeg_turbo']).startswith('3.')
    n = 0
    for name, mat, qualities, outs in golden_cases(golden_dir):
        assert len(qualities) == len(outs) >= 1
        for q, want in zip(qualities, outs):
            got = J.jpeg_roundtrip(mat, int(q))
            assert got.shape == want.shape and (got == want).all(), (name, int(q))
            n += 1
    assert n >= 250


def test_goldens_cover_the_issue_space(golden_dir):
    names = [name for name, *_ in golden_cases(golden_dir)]
    shapes = {tuple(int(v) for v in n.split('_')[0].split('x')[:2]) for n in names}
    assert {(h % 16, w % 16) for h, w in shapes} >= {(0, 0), (1, 1), (7, 5), (8, 8), (9, 9), (15, 1), (1, 12), (12, 1)}
    assert any(max(s) >= 1024 for s in shapes)
    assert {n.split('_')[1] for n in names} == {'random', 'gradient', 'saturated', 'asymmetric'}
    assert {n.split('_')[0].split('x')[2] for n in names} == {'1', '3'}
    # every quality of the issue's list at every shape up to 97 x 141, and all of them together
    per_shape = {}
    for name, _, qualities, _ in golden_cases(golden_dir):
        per_shape.setdefault(name.rsplit('x', 1)[0], set()).update(int(q) for q in qualities)
    every = {1, 2, 10, 24, 25, 49, 50, 51, 75, 95, 100}
    assert set().union(*per_shape.values()) == every
    assert all(per_shape[s] == every for s in per_shape if s not in ('256x256', '1031x23'))
    # the channel order matters on the asymmetric case: swapping B and R changes the result
    for name, mat, qualities, outs in golden_cases(golden_dir):
        if name == '97x141x3_asymmetric':
            swapped = J.jpeg_roundtrip(np.ascontiguousarray(mat[..., ::-1]), int(qualities[-1]))[..., ::-1]
            assert (swapped != outs[-1]).any()


def test_restatement_equals_pillow_on_seeded_random_cases():
    pytest.importorskip('PIL')
    rng = np.random.default_rng(7)
    for i in range(200):
        h, w = (int(v) for v in rng.integers(1, 120 if i % 10 else 400, 2))
        q = int(rng.integers(0, 101))
        gray = bool(rng.random() < 0.3)
        shape = (h, w) if gray else (h, w, 3)
        kind = i % 3
        if kind == 0:
            mat = rng.integers(0, 256, shape, dtype=np.uint8)
        elif kind == 1:
            mat = (rng.integers(0, 2, shape) * 255).astype(np.uint8)
        else:
            base = rng.integers(0, 256, ((h + 7) // 8, (w + 7) // 8) + shape[2:])      # flat 8 x 8 patches with a little noise
            mat = np.clip(np.repeat(np.repeat(base, 8, 0), 8, 1)[:h, :w] + rng.integers(-10, 11, shape), 0, 255).astype(np.uint8)
        got, want = J.jpeg_roundtrip(mat, q), J.pillow_roundtrip(mat, q)
        assert (got == want).all(), (i, shape, q)


def test_quant_tables_equal_the_dqt_segments_pillow_writes():
    PIL = pytest.importorskip('PIL.Image')
    for q in range(0, 101):
        buf = io.BytesIO()
        PIL.fromarray(np.zeros((8, 8, 3), np.uint8), 'RGB').save(buf, 'JPEG', quality=q)
        tables = PIL.open(io.BytesIO(buf.getvalue())).quantization
        luma, chroma = J.quant_tables(q)
        assert list(tables[0]) == list(luma) and list(tables[1]) == list(chroma), q
    assert all((a == b).all() for a, b in zip(J.quant_tables(0), J.quant_tables(1)))


def test_header_declares_and_library_exports_the_jpeg_entry_points():
    text = open(os.path.join(ROOT, 'include', 'vkx.h')).read()
    names = ('vkx_jpeg_roundtrip_u8', 'vkx_jpeg_roundtrip_u8_dev')
    for name in names:
        assert re.search(r'\bint\s+' + name + r'\s*\(', text), name
    from vkit_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    handle = ctypes.CDLL(_native.LIB_PATH)
    for name in names:
        assert hasattr(handle, name), name
        assert name in _native.EXPORTED_SYMBOLS
    assert callable(_native.jpeg_roundtrip)


def test_out_of_path_accepts_device_everywhere(monkeypatch):
    """'device' is a third behaviour next to 'pass_through' and 'raise' (which stay as they are); no GPU is touched here."""
    from vkit_amd.mechanism.distortion.photometric import opt
    from vkit_amd.mechanism.distortion_policy import random_distortion_factory
    assert opt.OUT_OF_PATH_OPERATORS == ('jpeg_quality',)
    with opt.out_of_path('device'):
        assert opt.out_of_path_behaviour() == 'device'
    assert opt.out_of_path_behaviour() == 'pass_through'
    monkeypatch.setenv('VKX_OUT_OF_PATH', 'device')
    assert opt.out_of_path_behaviour() == 'device'
    monkeypatch.delenv('VKX_OUT_OF_PATH')
    with pytest.raises(ValueError):
        opt.out_of_path('gpu')
    assert random_distortion_factory.create(None, out_of_path='device').out_of_path == 'device'
