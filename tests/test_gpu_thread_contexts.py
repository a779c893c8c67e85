"""One context per thread ("Threads / processes"): four threads with a context each enter the library together,
and two contexts share one thread, and every result equals a reference computed serially beforehand.  tests/thread_contexts.py
holds the families, the seeds, the rotation and the scenario; tests/test_thread_contexts_plan.py checks its lists on the CPU.

* ONE child process (the process-wide one-time work happens once per process): phase A, the first calls of the five families with
  one-time state behind a barrier; phase B, fifteen families rotated over the four threads, twice, on device-resident inputs;
  phase C, the thread-local refusal text, resident mode and default contexts.  The child prints one report line; the tests assert
  zero failures and the exact number of comparisons thread_contexts.planned() counts, so a phase that ran nothing fails.
* in this process: contexts A and B on one thread, the phase B families queued alternately with no synchronisation in between,
  both orders, and A's results against A alone.

Measured on an MI355X: the child 0.69 s, its start included (the scenario with its serial references 0.43 s); the three tests
together 1.5 s.
"""
import functools
import json
import os
import subprocess
import sys
import time

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import thread_contexts as T  # noqa: E402

pytestmark = pytest.mark.gpu

# tests/test_thread_contexts_plan.py checks them against the lists without a GPU
PLANNED = {'A': 36, 'B': 168, 'C': 14}
PLANNED_INTERLEAVED = 126
CHILD_TIMEOUT = 60       # seconds: ten times the 0.69 s measured on an MI355X is 7, below the floor of 60


@functools.lru_cache(maxsize=None)
def _child():
    """the report of the one child: {'compared': {phase: n}, 'declined', 'failures', 'n_failures', 'phase_c', 'seconds'}"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import sys; sys.path.insert(0, 'tests'); import thread_contexts; thread_contexts.child_main()"
    t0 = time.perf_counter()
    out = subprocess.run([sys.executable, '-c', code], cwd=root, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith(T.SENTINEL)]
    assert out.returncode == 0 and len(lines) == 1, out.stdout[-4000:] + out.stderr[-4000:]
    report = json.loads(lines[0][len(T.SENTINEL):])
    print(f'four-thread child, {time.perf_counter() - t0:.2f} s (scenario {report["seconds"]} s): compared {report["compared"]}, '
          f'declined poisson images {report["declined"]}, failures {report["n_failures"]}')
    return report


def test_four_threads_four_contexts_match_their_references():
    report = _child()
    assert report['n_failures'] == 0, '\n'.join(report['failures'])
    assert report['compared'] == PLANNED


def test_thread_local_state_is_per_thread():
    phase_c = _child()['phase_c']
    errors = phase_c['last_error']
    assert T.REFUSAL in errors[0], errors
    assert all(text is not None and T.REFUSAL not in text for text in errors[1:]), errors
    assert phase_c['resident_kind'] == {'1': 'DevArray', '2': 'ndarray'}
    assert phase_c['default_ctx_distinct'] == T.THREADS


def test_two_contexts_interleaved_on_one_thread():
    from vkit_amd import _native as N
    names = [f.name for f in T.FAMILIES_B]
    cases = [{f.name: f.make(T.seed_of(t, f, 1)) for f in T.FAMILIES_B} for t in (0, 1)]
    tally = T.Tally('one thread')
    a, b = N.Context(N.default_device()), N.Context(N.default_device())
    try:
        alone = T.interleave(N, a, None, cases[0], None, tally, 'A alone')
        a_first = T.interleave(N, a, b, cases[0], cases[1], tally, 'A then B')
        b_first = T.interleave(N, b, a, cases[1], cases[0], tally, 'B then A')
        a_second = T.interleave(N, a, None, cases[0], None, tally, 'A alone again')      # (what B then A left on A)
    finally:
        a.close()
        b.close()
    assert not tally.failures, '\n'.join(tally.failures[:40])
    print(f'interleaved: {tally.compared["B"]} comparisons, declined poisson images {tally.declined}')
    assert tally.compared['B'] == PLANNED_INTERLEAVED
    # A's results do not depend on B having run between its calls
    for got in (a_first, a_second):
        assert sorted(got) == sorted(names)
        for name in names:
            assert len(got[name]) == len(alone[name])
            for x, y in zip(got[name], alone[name]):
                if not isinstance(y, T.Declined):
                    assert T.same(x, y) is None, (name, T.same(x, y))
    assert sorted(b_first) == sorted(names)
