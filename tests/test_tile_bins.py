"""The host-side tile bins of vkit_amd/csrc/vkx_tile_bins.h -- the CSR builder of quad_interp.hip, region_label.hip and
image_combine.hip, and the per-box tile prefix of char_mask.hip and char_heatmap.hip -- on their own, on the CPU.

tools/tile_bins_check.cpp includes the header alone (plain C++17, no HIP).  Over seeded random planes from 1 x 1 to 300 x 300, the
three tile shapes in use (32 x 8, 32 x 32, 64 x 16) and 0 .. 200 rectangles, some widened and clamped, some behind a keep
predicate, it checks start[0] == 0, a monotone start, start[n_tiles] == the length of the list, and every tile's list against a
brute-force test of every (tile, item) pair; then the bound (exactly `bound` pairs pass, one more is refused, and a refused pass
has seen bound + 1 kept pairs, counted in the callable); then the box prefix against direct sums and its refusal at 2^31 tiles.
Two builds with the host compiler:
  sanitized   -O1 -g -fsanitize=address,undefined: exit 0, no sanitizer report, every check held.
  plain       -O2: the same checks at the optimisation level nearest the library's.
A stand-alone program: nothing here loads a sanitizer into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, 'tools', 'tile_bins_check.cpp')
CHECKS = 9           # lines '<check>: 0 of N mismatches' the program prints


@pytest.fixture(scope='module')
def cxx():
    found = shutil.which(os.environ.get('CXX', 'g++')) or shutil.which('c++') or shutil.which('clang++')
    assert found, 'no host C++ compiler'
    return found


def _build(cxx, out_dir, name, flags):
    exe = str(out_dir / name)
    proc = subprocess.run([cxx, *flags, '-std=c++17', '-Wall', '-o', exe, SOURCE], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    return exe


def _all_checks_hold(stdout):
    lines = stdout.splitlines()
    held = [ln for ln in lines if ': 0 of ' in ln]
    return len(held) == CHECKS and lines[-1] == 'all checks hold'


def test_bins_under_address_and_ub_sanitizers(cxx, tmp_path):
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    linked = subprocess.run([cxx, '-fsanitize=address,undefined', '-o', str(tmp_path / 'probe'), str(probe)], capture_output=True,
                            text=True)
    if linked.returncode != 0:
        pytest.skip(f'{cxx} cannot link with -fsanitize=address,undefined: {linked.stderr.strip()[-200:]}')
    exe = _build(cxx, tmp_path, 'tile_bins_check_san', ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'])
    env = dict(os.environ, ASAN_OPTIONS='halt_on_error=1 exitcode=66', UBSAN_OPTIONS='halt_on_error=1 print_stacktrace=1')
    proc = subprocess.run([exe], env=env, capture_output=True, text=True)
    assert proc.returncode == 0, (proc.returncode, proc.stdout[-2000:] + proc.stderr[-4000:])
    assert 'Sanitizer' not in proc.stderr and 'runtime error' not in proc.stderr, proc.stderr[-4000:]
    assert _all_checks_hold(proc.stdout), proc.stdout


def test_bins_at_O2(cxx, tmp_path):
    exe = _build(cxx, tmp_path, 'tile_bins_check', ['-O2'])
    proc = subprocess.run([exe], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert _all_checks_hold(proc.stdout), proc.stdout
