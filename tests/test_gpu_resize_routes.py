"""Both device forms of the CUBIC / LANCZOS4 resize (vkit_amd/csrc/resize.hip: the separable k_resize_sep, the direct
k_resize_taps_u8 / _f32) against oracle.resize, bit for bit, at the shapes where the host's choice between them switches, and the
near misses of the other decisions of the routing rule.  tests/resize_routes.py holds the geometry lists, the sources and the
comparison; tests/test_resize_routes_shapes.py checks on the CPU that the lists sit where they claim to.

* in this process (default routing): bands of source heights around the 24 | 25 row switch between the two uint8 instances of
  the separable kernel and the 40 | 41 row switch to the direct kernels, for either tap count, along y and transposed; destination
  widths on the tile and 4-pixel-group edges; sources of fewer pixels than taps; enlargements, the identity, shrinks around 2x; the
  LANCZOS4 NaN-coefficient geometries; and for all seven codes the exact half missed on one axis, AREA with one integer factor,
  unequal factors, factor 1 and a large factor, NEAREST_EXACT on odd and even sources.  Sources: random uint8 x 1 / 3 / 4
  channels, a 0 / 1 mask, random float32, all 255, 0 / 255 stripes of period 2, 3, 4 along either axis, float32 with inf, -inf,
  NaN and -0.0.
* in ONE child process with VKX_RESIZE_DIRECT=1 (read once per process): the same sweep and the same random cases for CUBIC and
  LANCZOS4, every call in the direct form -- enlargements, identity, clipped sources and the tile edges it never sees otherwise.
* 8000 seeded random geometries (sizes 1 .. 160, every second dh around sh / 2), a count and not a time budget.

The only combination skipped is INTER_AREA that enlarges, which must raise VkxError; every test asserts its compared and skipped
counts against the numbers below.  Measured on an MI355X: the sweep in this process (5876 comparisons) 1.2 s, the 8000 random
cases (7240 comparisons) 1.6 s, the child (2964 + 2244 comparisons, its start included) 2.4 s.
"""
import functools
import json
import os
import subprocess
import sys
import time

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resize_routes as R  # noqa: E402

pytestmark = pytest.mark.gpu

# (compared, skipped): tests/test_resize_routes_shapes.py checks them against the lists without a GPU
SWEEP_ALL = (5876, 403)
SWEEP_TAPS = (2964, 0)
RANDOM_ALL = (7240, 760)
RANDOM_TAPS = (2244, 0)


def test_both_forms_equal_the_oracle_in_this_process():
    assert not os.environ.get('VKX_RESIZE_DIRECT'), 'this test is about the default routing'
    t0 = time.perf_counter()
    compared, skipped = R.run_sweep(R.ALL_CODES)
    print(f'sweep, default routing: {compared} compared, {skipped} skipped, {time.perf_counter() - t0:.2f} s')
    assert (compared, skipped) == SWEEP_ALL


@functools.lru_cache(maxsize=None)
def _direct_child():
    """the report of the one forced-direct child: {'sweep': [compared, skipped, seconds] or failures, 'random': the same}"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import sys; sys.path.insert(0, 'tests'); import resize_routes; resize_routes.child_main()"
    t0 = time.perf_counter()
    out = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, VKX_RESIZE_DIRECT='1'), cwd=root, capture_output=True,
                         text=True, timeout=300)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith(R.SENTINEL)]
    assert out.returncode == 0 and len(lines) == 1, out.stdout[-4000:] + out.stderr[-4000:]
    print(f'forced-direct child, {time.perf_counter() - t0:.2f} s: {lines[0][:300]}')
    return json.loads(lines[0][len(R.SENTINEL):])


def test_direct_form_equals_the_oracle_everywhere():
    part = _direct_child()['sweep']
    assert isinstance(part, list), part
    assert tuple(part[:2]) == SWEEP_TAPS


def test_random_geometries():
    t0 = time.perf_counter()
    compared, skipped = R.run_random()
    print(f'random geometries, default routing: {compared} compared, {skipped} skipped, {time.perf_counter() - t0:.2f} s')
    assert (compared, skipped) == RANDOM_ALL
    part = _direct_child()['random']
    assert isinstance(part, list), part
    assert tuple(part[:2]) == RANDOM_TAPS
