"""The host replay of a sample-trace row's summation order (tests/tracereplay.py) past one value per thread: the device tests
hold the rows of sets of more than 1 024 loci against it with == (tests/test_gpu_trace_tails.py), so it is held here against
the exact sum, against a tree written out value by value, and against itself part by part."""
import math

import numpy as np
import pytest

from tracereplay import replay_sum, replay_parts, any_order_bound

SIZES = (1, 2, 1023, 1024, 1025, 2049, 2500)


def mixed(n, seed):
    """n doubles of both signs over twelve orders of magnitude"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)


def pairwise_tree(values, threads):
    """sh[t] += sh[t + w] for t < w, w = threads/2 ... 1 on one value per thread (the rest 0.0), in plain Python floats"""
    sh = [float(x) for x in values] + [0.0] * (threads - len(values))
    w = threads // 2
    while w > 0:
        for t in range(w):
            sh[t] = sh[t] + sh[t + w]
        w //= 2
    return sh[0]


@pytest.mark.parametrize("n", SIZES)
def test_replay_sum_is_within_the_any_order_bound_of_the_exact_sum(n):
    """math.fsum is the exact sum rounded once.  No value passes through more than ceil(n/1024) + 10 additions here, so the
    replay's error is far inside n 2^-53 sum|x| for the large n and one rounding (fsum's own) at n <= 2"""
    v = mixed(n, 100 + n)
    assert n <= 2 or np.abs(v).max() / np.abs(v).min() > 1e6
    assert abs(replay_sum(v) - math.fsum(v)) <= any_order_bound(v)
    assert abs(replay_sum(v, threads=512) - math.fsum(v)) <= any_order_bound(v)


@pytest.mark.parametrize("n", [k for k in SIZES if k <= 1024])
def test_with_one_value_per_thread_the_replay_is_the_plain_pairwise_tree(n):
    v = mixed(n, 200 + n)
    assert replay_sum(v) == pairwise_tree(v, 1024)
    if n <= 4:
        assert replay_sum(v, threads=4) == pairwise_tree(v, 4)


def test_a_thread_adds_its_values_in_turn_before_the_tree():
    """n = 1 025: thread 0 adds values 0 and 1 024, everyone else one; 2 500: threads 0 .. 451 add three, the rest two —
    the tree then runs over the threads' sums"""
    for n in (1025, 2049, 2500):
        v = mixed(n, 300 + n)
        sums = []
        for t in range(1024):
            acc = 0.0
            for k in range(t, n, 1024):
                acc = acc + float(v[k])
            sums.append(acc)
        assert len(range(0, n, 1024)) == -(-n // 1024) and len(range(1023, n, 1024)) == n // 1024
        assert replay_sum(v) == pairwise_tree(sums, 1024)
    assert len(range(451, 2500, 1024)) == 3 and len(range(452, 2500, 1024)) == 2


def test_replay_parts_adds_the_parts_sums_in_part_order():
    a, b, c = mixed(1025, 1), mixed(70, 2), mixed(6, 3)
    assert replay_parts([a]) == replay_sum(a)
    assert replay_parts([a, b]) == float(np.float64(replay_sum(a)) + replay_sum(b))
    assert replay_parts([a, b, c]) == float((np.float64(replay_sum(a)) + replay_sum(b)) + replay_sum(c))
