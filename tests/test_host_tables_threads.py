"""The process-wide host tables of vkit_amd/csrc/vkx_host_tables.h -- OpenCV's SinTable and the PCG64 jump constants -- entered
from eight threads at once, on the CPU.

tools/host_tables_check.cpp includes the header alone (plain C++17, no HIP), releases eight std::threads together, lets each make
its first call to both accessors and checksum what it reads, then checks the values: SinTable against sin itself, the jump
constants against the generator stepped one draw at a time.  Two builds with the host compiler:
  sanitized   -O1 -g -fsanitize=thread, run three times with halt_on_error: exit 0 and no ThreadSanitizer report.  On the tables
              as they were before the header (a static array behind a plain bool) this build reports the race in the builder and
              in the reader: profiles/host_tables_tsan.md keeps both outputs.
  plain       -O2, once: the value checks at the optimisation level nearest the library's.
A stand-alone program: nothing here loads a sanitizer into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, 'tools', 'host_tables_check.cpp')
CHECKS = 8           # lines '<check>: 0 of N mismatches' the program prints


@pytest.fixture(scope='module')
def cxx():
    found = shutil.which(os.environ.get('CXX', 'g++')) or shutil.which('c++') or shutil.which('clang++')
    assert found, 'no host C++ compiler'
    return found


def _build(cxx, out_dir, name, flags):
    exe = str(out_dir / name)
    proc = subprocess.run([cxx, *flags, '-std=c++17', '-pthread', '-Wall', '-o', exe, SOURCE], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    return exe


def _all_checks_hold(stdout):
    lines = stdout.splitlines()
    held = [ln for ln in lines if ': 0 of ' in ln]
    return len(held) == CHECKS and lines[-1] == 'all checks hold'


def test_eight_threads_under_thread_sanitizer(cxx, tmp_path):
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    linked = subprocess.run([cxx, '-fsanitize=thread', '-pthread', '-o', str(tmp_path / 'probe'), str(probe)], capture_output=True,
                            text=True)
    if linked.returncode != 0:
        pytest.skip(f'{cxx} cannot link with -fsanitize=thread: {linked.stderr.strip()[-200:]}')
    exe = _build(cxx, tmp_path, 'host_tables_check_tsan', ['-O1', '-g', '-fsanitize=thread'])
    env = dict(os.environ, TSAN_OPTIONS='halt_on_error=1 exitcode=66')
    for run in range(3):
        proc = subprocess.run([exe], env=env, capture_output=True, text=True)
        assert proc.returncode == 0, (run, proc.returncode, proc.stdout[-2000:] + proc.stderr[-4000:])
        assert 'ThreadSanitizer' not in proc.stderr, (run, proc.stderr[-4000:])
        assert _all_checks_hold(proc.stdout), (run, proc.stdout)


def test_values_at_O2(cxx, tmp_path):
    exe = _build(cxx, tmp_path, 'host_tables_check', ['-O2'])
    proc = subprocess.run([exe], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert _all_checks_hold(proc.stdout), proc.stdout
