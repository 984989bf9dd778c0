"""The generic and the big-tree sampler share ONE launch loop of an iteration (csrc/gsampler_host.hpp: gs_iterate, through
sampler_step / sampler_eval).  This test holds that loop to what the two separate loops did before they were joined:
tests/golden/launch_loop.json was recorded on the MI355X at the commit before the join (tests/golden/make_golden_launch_loop.py).

Every case runs 6 iterations as iterate(1), iterate(2), iterate(3) and then reads: summary() (launches, proposals, accepted),
gibbs_counters(), the rate and the heredity counters — compared as integers — and taus, thetas, total lnL, rates, their mean
and the heredity scalars (the trace's rows where one is on) — compared bit for bit, as hex floats.  The margin is zero because
the join moved host code only: same kernels, same launch order, same order of draws.  It is not a measured tolerance.  A float the
generator could not reproduce between two runs of the same code is not in the fixture (its name is under "unreproducible")."""
import json
import os

import numpy as np
import pytest

import bpp_amd
import heredity as HD
import locusrates as LR
import shapes
import tape

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_loop.json")
SEED = 31
CALLS = (1, 2, 3)
EVERY = 3


def _set(name):
    """-> (the dict locusrates.configure takes, the sampler's options, scale buffers, kind())"""
    if name == "gtr-g4":                           # 12 GTR+Gamma4 8-tip loci: the packing's kernels, never chained
        return LR.case("b", 12), {}, False, "generic"
    if name == "jc-chained":                       # 40 JC69 4-tip loci, one of 65 patterns: GAGE + GSPR in one launch
        return dict(shapes.case("handover-65"), model="jc69"), dict(chain=True), False, "generic"
    if name == "jc-unchained":
        return dict(shapes.case("handover-65"), model="jc69"), dict(chain=False), False, "generic"
    if name == "lg-g4":                            # 8 LG+Gamma4 6-tip loci: the 20-state records
        return LR.case("d", 8), {}, False, "generic"
    if name == "big-forced":                       # the big-tree sampler on loci the generic one would take
        return LR.case("b", 12), dict(implementation="big"), False, "big"
    assert name == "big-17"                        # 17 tips, scale buffers
    return dict(shapes.case("big-17-30"), model="jc69"), {}, True, "big"


SETS = ("gtr-g4", "jc-chained", "jc-unchained", "lg-g4", "big-forced", "big-17")
# (set, moves, the moves after MIX on, trace): both move sets with the tail off and on, then the tail once more under a trace
CASES = [(s, m, t, False) for s in SETS for m in ("uniform", "program") for t in (False, True)] + [(s, "program", True, True) for s in SETS]


def case_id(name, moves, tail, trace):
    return f"{name}-{moves}-{'tail' if tail else 'plain'}" + ("-trace" if trace else "")


def hexes(values):
    return [float(x).hex() for x in np.asarray(values, dtype=float).ravel()]


def run_case(name, moves, tail, trace):
    """-> (integers, floats as hex) of the case after its 6 iterations"""
    c, options, scaling, kind = _set(name)
    n = len(c["data"])
    eng = bpp_amd.Engine(0)
    dev = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, c["data"], scaling), c["data"], seed=SEED, **options)
    if tail:          # heredity, rates and their mean everywhere; frequencies, exchangeabilities and alpha where the loci have them
        HD.configure(dev, c, moves, False, subst=c["model"] == "gtr", rates=True, scalars=HD.start_scalars(n))
    else:
        LR.configure(dev, c, moves, False, ft=None)
    dev.initialize()
    assert dev.kind() == kind
    if trace:
        dev.set_trace(EVERY, 64)
    for k in CALLS:
        dev.iterate(k)
    s = dev.summary()
    rates = dev.locusrate_counters()
    ints = dict(launches=s["launches"], proposals=s["proposals"], accepted=s["accepted"], gibbs=list(dev.gibbs_counters()),
                mui=list(rates["mui"]), mubar=list(rates["mubar"]), heredity=list(dev.heredity_counters()))
    mui, mubar = dev.get_locus_rates()
    floats = dict(taus=hexes(dev.taus()), thetas=hexes(dev.thetas()), total_lnl=hexes([s["total_lnl"]]), rates=hexes(mui), mubar=hexes([mubar]),
                  scalars=hexes(dev.get_heredity()))
    if trace:
        rows = dev.trace()
        ints["trace_iterations"] = [int(x) for x in rows["iteration"]]
        floats.update(trace_lnl=hexes(rows["lnl"]), trace_taus=hexes(rows["taus"]), trace_thetas=hexes(rows["thetas"]))
    dev.close()
    eng.close()
    return ints, floats


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name,moves,tail,trace", CASES, ids=[case_id(*c) for c in CASES])
def test_launch_loop_equals_the_loops_before_the_join(golden, name, moves, tail, trace):
    want = golden["cases"][case_id(name, moves, tail, trace)]
    ints, floats = run_case(name, moves, tail, trace)
    print(f"[launch-loop] {case_id(name, moves, tail, trace)}: {ints}")
    assert ints == want["ints"]
    assert ints["proposals"] > ints["accepted"] > 0
    if tail:
        assert ints["mui"][0] == ints["heredity"][0] == sum(CALLS)*len(floats["rates"]) and ints["mubar"][0] == sum(CALLS)
    if trace:
        assert ints["trace_iterations"] == list(range(EVERY, sum(CALLS) + 1, EVERY))
    assert set(want["floats"]) | set(want["unreproducible"]) == set(floats)
    for key, value in want["floats"].items():
        assert floats[key] == value, key
