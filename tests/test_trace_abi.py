"""CPU side of the sample trace (bpa_sampler_set_trace / _trace_width / _trace_read): the three calls are declared in
include/bpp_amd.h, exported by the library and bound by bpp_amd.api; and the host replay of a row's summation order
(tests/tracereplay.py, which tests/test_gpu_trace.py holds the device's rows against) does what the header says."""
import os
import re

import numpy as np

import bpp_amd
from bpp_amd import api
from tracereplay import replay_sum, replay_parts, any_order_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bpa_sampler_set_trace", "bpa_sampler_trace_width", "bpa_sampler_trace_read")


def test_the_three_calls_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "bpp_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = bpp_amd.lib()
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", code), f"{n} is not declared in include/bpp_amd.h"
        assert hasattr(L, n), f"{n} is not exported"
        assert n in api.EXPORTED
    assert L.bpa_sampler_trace_read.restype is api.C.c_long
    for m in ("set_trace", "trace", "trace_read", "trace_width"):
        assert callable(getattr(bpp_amd.Sampler, m))
    # the header says what a row is and in which order its lnL is added up
    for words in ("[iteration, lnL, tau[0 .. npop), theta[0 .. npop)]", "t + 1024", "sh[t] += sh[t + w]", "Several ranks"):
        assert words in src, words


def test_replay_follows_the_documented_order_on_a_hand_computed_example():
    """Loci in three threads of the 1 024: n = 1027, so thread 0 adds values 0 and 1024, thread 1 values 1 and 1025, thread 2
    values 2 and 1026, every other thread one value (0.0 here).  The tree then gives ((s0 + s2) + s1): sh[0] += sh[2] at w = 2,
    sh[1] += sh[3] (0.0), sh[0] += sh[1] at w = 1.  With s0 = 1e16 + 1 = 1e16 (1 is below half an ulp of 2), s2 = -1e16 + 3 and
    s1 = 1 + 0.5 that is (1e16 + (-1e16 + 3)) + 1.5; -1e16 + 3 rounds to -1e16 + 4 (ulp 2, tie to even), so the result is 5.5 —
    where the sum in index order gives ((((1e16 + 1) - 1e16) + 1) + 0.5) + 3 = 4.5."""
    v = np.zeros(1027)
    v[0], v[1024] = 1e16, 1.0
    v[1], v[1025] = 1.0, 0.5
    v[2], v[1026] = -1e16, 3.0
    s0, s1, s2 = 1e16 + 1.0, 1.0 + 0.5, -1e16 + 3.0
    assert s0 == 1e16 and s2 == -1e16 + 4.0
    assert replay_sum(v) == (s0 + s2) + s1 == 5.5
    seq = 0.0
    for x in v:
        seq += x
    assert seq == 4.5                                    # the order matters on this example
    # the same shape with 4 threads, by hand: threads hold (1+5, 2+6, 3, 4); tree: (6+3, 8+4) -> 9 + 12
    assert replay_sum([1, 2, 3, 4, 5, 6], threads=4) == 21.0
    assert replay_sum([], threads=4) == 0.0 and replay_sum([-0.0]) == 0.0
    assert replay_parts([[1e16, 1.0], [-1e16], [1.0]]) == (np.float64(1e16) + -1e16) + 1.0 == 1.0
    assert any_order_bound([1.0, -2.0, 4.0]) == 3 * 2.0 ** -53 * 7.0
