"""The plan of tests/thread_contexts.py, checked on the CPU: the comparison counts the GPU tests assert, the families behind
every one-time state of phase A, the rotation of phase B, the seeds, and the references themselves (they are computed without a
GPU, so a family whose reference cannot be built fails here first)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import thread_contexts as T  # noqa: E402
import test_gpu_thread_contexts as G  # noqa: E402


def test_planned_counts_are_the_constants_the_gpu_tests_assert():
    assert T.planned() == G.PLANNED == {'A': 36, 'B': 168, 'C': 14}
    assert T.planned_interleaved() == G.PLANNED_INTERLEAVED == 126
    per_thread_a = sum(f.count for f in T.FAMILIES_A)
    per_thread_b = sum(f.count for f in T.FAMILIES_B)
    assert (per_thread_a, per_thread_b) == (9, 21)
    assert T.planned()['A'] == 4 * per_thread_a and T.planned()['B'] == 4 * 2 * per_thread_b
    assert G.CHILD_TIMEOUT >= 60


def test_phase_a_covers_the_five_one_time_states():
    names = [f.name for f in T.FAMILIES_A]
    assert sorted(names) == sorted(T.ONE_TIME_STATE) and len(names) == 5
    text = ' '.join(T.ONE_TIME_STATE.values())
    for state in ('SinTable', 'jump tables', 'NpTabs', "poisson.hip's tables", 'HSV tables', 'resize table cache'):
        assert state in text, state
    # the families of phase A run again in phase B, warm
    assert T.FAMILIES_B[:len(T.FAMILIES_A)] == T.FAMILIES_A
    assert len(T.FAMILIES_B) == 15 and len({f.name for f in T.FAMILIES_B}) == 15


def test_rotation_puts_every_family_on_every_thread_and_none_on_two_at_once():
    n = len(T.FAMILIES_B)
    assert T.THREADS <= n
    for t in range(T.THREADS):
        assert sorted(T.rotation(s, t) for s in range(n)) == list(range(n))
    for s in range(n):
        assert len({T.rotation(s, t) for t in range(T.THREADS)}) == T.THREADS


def test_every_case_has_its_own_seed_and_its_own_reference():
    cases = T.expectations()
    assert len(cases) == T.THREADS * (len(T.FAMILIES_A) + T.ROUNDS_B * len(T.FAMILIES_B) + 1)
    seeds = [tuple(T.seed_of(t, f, r)) for t in range(T.THREADS) for f in T.FAMILIES_B for r in range(T.ROUNDS_B + 2)]
    assert len(set(seeds)) == len(seeds)
    by_name = {f.name: f for f in T.FAMILIES_B}
    for (t, name, r), case in cases.items():
        assert len(case['want']) == by_name[name].count, (t, name, r)
    # no two cases of a family expect the same bytes: a result that lands in another context is a mismatch
    for f in T.FAMILIES_B:
        firsts = [case['want'][0] for (t, name, r), case in cases.items() if name == f.name]
        blobs = {np.asarray(w).tobytes() for w in firsts}
        assert len(blobs) == len(firsts), f.name
        assert all(np.asarray(w).any() for w in firsts), f.name       # and none is an empty plane


def test_same_tells_arrays_apart():
    a = np.arange(12, dtype=np.uint8).reshape(3, 4)
    assert T.same(a.copy(), a) is None
    assert T.same(a.astype(np.int16), a) and T.same(a.reshape(4, 3), a) and T.same(None, a)
    b = a.copy()
    b[2, 1] += 1
    assert '1 values differ, first at (2, 1)' in T.same(b, a)
    assert T.same({'s': 1}, {'s': 1}) is None and T.same({'s': 1}, {'s': 2})
    tally = T.Tally('x')
    tally.compare('B', T.NpPoisson, [T.Declined(4, True)] * 2, [a, {}])
    assert tally.declined == 1 and tally.compared == {'B': 2} and not tally.failures
    tally.compare('B', T.NpPoisson, [T.Declined(0, True)] * 2, [a, {}])
    tally.compare('B', T.ColorShift, [b], [a])
    tally.compare('B', T.ColorShift, [], [a])
    assert len(tally.failures) == 4
