"""The program's THETA / TAU / MIX decisions are stated ONCE, in include/bpp_amd_priors.h (a00_prog_*): the C host driver
(csrc/host/a00_driver.c: theta_step_gibbs, tau_step, mix_step) and the generic sampler's host_decisions form
(csrc/gsampler_host.hpp: gs_prog_theta / _tau / _mix) call the same functions.  This test holds the host driver to what its own
copy of those statements did before they moved: tests/golden/prog_decisions_host.json (the integers) and .npz (the doubles, as
recorded: compared through their 64 bits) were taken at the commit before the move (tests/golden/make_golden_prog_decisions.py
host).  GPU twin, for the sampler's side: tests/test_gpu_prog_decisions_sampler.py.

hostdrv.prior_driver (lnL = 0): the decisions alone steer the chain.  12 loci on the 4-species tree, two sequences a species
(tests/test_invgamma_host.py's _several) or one (no tip population has a theta), 40 iterations.  After EVERY iteration: every tau,
every theta and the sum of the trees' logpr, bit for bit (a mismatch is shown as hex floats); at the end a00_counters,
a00_gibbs_counters and the heredity counters as integers.  The driver is deterministic: the generator ran every case twice and nothing is left out; the margin is zero by construction.  A 1-thread and
a 4-thread row of the same case are equal to each other.

The NaN branches:
  overflow  locus 0's heredity scalar 1e-6: |T2h/h| >= 256, theta_sums reports the sums unusable (run_ok = 0) and every THETA, TAU
            and MIX decision of the run is NaN (A00_DECLOG=1: all 440 lines say `lnacc nan`); no new API needed.
  a failed fit cannot be started without new API: a00_theta_conditional returned a fit for every (a, b, k, T) tried (a 1.2 .. 3,
            b 0.1 .. 1000, k 0 .. 40, T 1e-4 .. 1), and the driver has no call that sets k or T.  `widetheta`, a gamma(2, 10) theta
            prior, was the attempt (no decision of it is NaN); it stays as one more gamma row."""
import json
import os

import numpy as np
import pytest

from bpp_amd import synth
import heredity as HD
import invgamma as IG

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prog_decisions_host.json")
ITERS = 40
NLOCI = 12
SEED = 23

# (shape, theta / tau prior kind, slide_prob, heredity scalars set, threads, variant)
CASES = [(sh, k, sl, h, t, "plain") for sh in ("4x2", "4x1") for k in ("gamma", "invgamma") for sl in (0.0, 0.1, 1.0) for h in (False, True) for t in (1, 4)]
CASES += [("4x2", k, 0.1, False, t, "flat-tau") for k in ("gamma", "invgamma") for t in (1, 4)]
CASES += [("4x2", "gamma", 0.1, False, t, "widetheta") for t in (1, 4)]
CASES += [("4x2", k, 0.1, True, t, "overflow") for k in ("gamma", "invgamma") for t in (1, 4)]
CASES += [("4x2", k, 0.1, False, t, "uniform") for k in ("gamma", "invgamma") for t in (1, 4)]          # accept()'s other branch


def case_id(shape, kind, slide, hered, threads, variant):
    return f"{shape}-{kind}-slide{slide:g}-{'hered' if hered else 'nohered'}-t{threads}-{variant}"


def row_id(shape, kind, slide, hered, threads, variant):
    """the fixture's key: a case without its thread count"""
    return f"{shape}-{kind}-slide{slide:g}-{'hered' if hered else 'nohered'}-{variant}"


_DATA = {}


def data_of(shape):
    """built once, never changed -> (data, stree, tip species)"""
    if shape not in _DATA:
        stree = synth.species_tree_arrays(4, 0.01)
        parent, tau0, thetas = stree
        sp = [0, 0, 1, 1, 2, 2, 3, 3] if shape == "4x2" else [0, 1, 2, 3]
        rng = np.random.default_rng(77)
        data = []
        for _ in range(NLOCI):
            l, r, t, rt = synth.msc_start_tree(sp, parent, tau0, thetas, rng)
            data.append(dict(seqs=["A"]*len(sp), left=l, right=r, times=t, root=rt))
        _DATA[shape] = (data, stree, sp)
    return _DATA[shape]


def run_case(shape, kind, slide, hered, threads, variant):
    """-> (integers, a row per iteration: taus, thetas, sum of logpr)"""
    data, stree, sp = data_of(shape)
    tau0 = stree[1]
    drv = IG.KindDriver(HD.prior_driver(data, seed=SEED))
    inv = kind == "invgamma"
    theta_prior = (3.0, 0.02, 0.008) if inv else (2.0, 10.0, 0.008) if variant == "widetheta" else (2.0, 200.0, 0.008)
    tau_prior = (0.0, 0.0) if variant == "flat-tau" else (3.0, 2.0*tau0[-1]) if inv else (3.0, 3.0/tau0[-1])
    IG.configure(drv, stree, [sp]*NLOCI, "uniform" if variant == "uniform" else "program", theta_prior=theta_prior, tau_prior=tau_prior,
                 finetune=(0.008, 0.008, 0.002, 0.5), kinds=(kind, kind))
    if variant != "uniform":
        drv.set_program_moves(True, slide)
    if hered:
        h = HD.start_scalars(NLOCI)
        if variant == "overflow":
            h[0] = 1e-6
        drv.set_heredity(h)
        if variant != "overflow":
            drv.set_heredity_move(0.6, 4.0, 4.0)
    drv.set_threads(threads)
    drv.initialize()
    rows = []
    for _ in range(ITERS):
        drv.iterate()
        rows.append(list(drv.taus()) + list(drv.thetas()) + [sum(drv.tree(i)["logpr"] for i in range(NLOCI))])
    ints = dict(counters=list(drv.counters()), gibbs=list(drv.gibbs_counters()), heredity=list(drv.heredity_counters()))
    drv.close()
    return ints, np.array(rows, dtype=np.float64)


def same_bits(got, want):
    """every double equal in all 64 bits; the first that is not, as hex floats"""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
    assert len(bad) == 0, (tuple(bad[0]), float(got[tuple(bad[0])]).hex(), float(want[tuple(bad[0])]).hex(), len(bad))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    with np.load(GOLDEN[:-5] + ".npz") as z:
        g["rows"] = {k: z[k] for k in z.files}
    return g


def test_the_fixture_has_one_row_for_all_thread_counts(golden):
    assert set(golden["cases"]) == {row_id(*c) for c in CASES}
    assert set(golden["rows"]) == set(golden["cases"]) and all(v.shape[0] == ITERS for v in golden["rows"].values())


@pytest.mark.parametrize("shape,kind,slide,hered,threads,variant", CASES, ids=[case_id(*c) for c in CASES])
def test_host_driver_decides_as_before_the_move(golden, shape, kind, slide, hered, threads, variant):
    rid = row_id(shape, kind, slide, hered, threads, variant)
    ints, rows = run_case(shape, kind, slide, hered, threads, variant)
    print(f"[prog-decisions-host] {case_id(shape, kind, slide, hered, threads, variant)}: {ints}")
    assert ints == golden["cases"][rid]
    same_bits(rows, golden["rows"][rid])
    p, a, _ = ints["counters"]
    assert p > a > 0
    gp, ga = ints["gibbs"]
    if variant == "uniform":
        assert (gp, ga) == (0, 0)
    elif slide == 1.0:
        assert (gp, ga) == (0, 0)                              # every THETA proposal slides
    elif variant == "overflow":
        assert gp > 0 and ga == 0                              # the sums are unusable: nothing of the program's moves is accepted
    elif kind == "invgamma":
        assert gp > 0 and ga == gp                             # the conditional itself: always accepted
    if slide == 0.0 and variant == "plain":
        assert gp == ITERS*(7 if shape == "4x2" else 3)        # 4x1: the tips' populations have no theta
