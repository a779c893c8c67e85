"""The cheaper forms of the hue round trip in vkit_amd/csrc/vkx_color.h, proven on every input on the CPU.

tools/hue_forms_check.cpp includes the header in its host mode (plain C++ fallbacks behind the device builtins), so the program
runs the source lines the kernels compile.  Built with the host compiler and -ffp-contract=off, as the library is:
  forward    all 2^24 (r, g, b): S, V and H mod 256 of rgb2hsv_full against the integer arithmetic of oracle/vkx_oracle.c
  backward   all 2^24 (H, S, V): hsv2rgb_packed against hsv2rgb_full
  roundtrip  hue_shift_packed over the all-triples image against oracle.color_shift_rgb (the oracle the GPU tests use)"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, 'tools', 'hue_forms_check.cpp')


@pytest.fixture(scope='module')
def checker(tmp_path_factory):
    cxx = shutil.which(os.environ.get('CXX', 'g++')) or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('hue_forms') / 'hue_forms_check')
    proc = subprocess.run([cxx, '-O2', '-std=c++17', '-ffp-contract=off', '-Wall', '-o', exe, SOURCE], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    return exe


def _run(exe, *args):
    proc = subprocess.run([exe, *args], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    return proc.stdout


def test_forward_every_rgb_triple(checker):
    assert 'forward: 0 mismatches' in _run(checker, 'forward')


def test_backward_every_hsv_triple(checker):
    assert 'backward: 0 mismatches' in _run(checker, 'backward')


@pytest.fixture(scope='module')
def all_triples():
    v = np.arange(256, dtype=np.uint8)
    return np.ascontiguousarray(np.stack(np.meshgrid(v, v, v, indexing='ij'), -1).reshape(4096, 4096, 3))


@pytest.mark.parametrize('delta', [0, 1, 37, 128, 255])
def test_round_trip_equals_the_oracle(checker, all_triples, tmp_path, delta):
    out = tmp_path / 'shifted.bin'
    _run(checker, 'roundtrip', str(delta), str(out))
    got = np.fromfile(out, np.uint8).reshape(all_triples.shape)
    out.unlink()
    want = O.color_shift_rgb(all_triples, delta)
    assert (got == want).all(), (delta, int((got != want).any(-1).sum()))
