"""Heredity scalars on the generic device sampler (bpa_sampler_set_heredity / bpa_sampler_set_heredity_move: the h_i of BPP's
'heredity = 1 a b' and 'heredity = 2 file' — gdensity_term, gstep2_body's lane groups, the THETA / TAU sum kernels, step mode
10 of gsm2::gstep2_kernel) against the C host driver on the same library, against a CPU recompute, against the priors, and
what the other samplers refuse.  CPU twin: tests/test_heredity_host.py; the program's posterior: tests/test_heredity_posterior.py."""
import numpy as np
import pytest

import bpp_amd
from bpp_amd import synth
import tape
import locusrates as LR
import heredity as HD
import shapes

pytestmark = pytest.mark.gpu


def _pair(c, seed, generic=False, **options):
    """(engine, engine loci of the device sampler, host driver, device sampler) on case c's data"""
    eng = bpp_amd.Engine(0)
    data = c["data"]
    loci_a = tape.make_engine_loci(eng, data)
    loci_b = tape.make_engine_loci(eng, data)
    host = HD.hip_driver(eng, loci_a, data, seed=seed)
    dev = bpp_amd.Sampler(eng, loci_b, data, seed=seed, implementation="generic" if generic else None, **options)
    return eng, loci_b, host, dev


# case, moves, iterations, options, the rate moves on as well
TRAJECTORIES = [
    ("a", "uniform", 5, None, False),                      # 70 loci forced generic: two workgroups of gstep_kernel; the chain launch
    ("a", "uniform", 5, dict(chain=False), False),          # ... and a launch per step
    ("a", "program", 3, None, False),                      # BPP's kernel, THETA / TAU / MIX decided on the device from the sums of T2h/h
    ("a", "program", 3, dict(host_decisions=True), False),        # ... and on the host
    ("b", "uniform", 5, None, False),                      # two part-batches, fuse_pm, the substitution moves after HRDT
    ("b", "program", 3, None, False),
    ("b", "uniform", 5, None, True),                       # ... with MUI and MUBAR
    ("c", "uniform", 5, None, False),                      # 16 tips: 32-lane groups
    ("c", "program", 3, None, False),
    ("b", "uniform", 5, dict(one_call=True), False),                # all iterations in one iterate call
]


@pytest.mark.parametrize("name,moves,iters,env,rates", TRAJECTORIES, ids=shapes.option_id)
def test_device_sampler_with_heredity_equals_host_driver(name, moves, iters, env, rates):
    """scalars log-uniform on (0.25, 2), HRDT on: same decisions, counters (the sampler's and HRDT's), trees and buffer indices
    as the host driver's hered_step and its densities at h_i theta; ages, taus, thetas and scalars to locusrates.walk's bars
    (1e-12 uniform — the scalars ==: h' = |h + ft_h (u - 1/2)| involves no libm —, 1e-9 with the program's moves), logpr to
    1e-11, total lnL to 1e-10"""
    c = LR.case(name)
    n = len(c["data"])
    subst = name == "b"
    env = dict(env or {})
    one_call = env.pop("one_call", False)
    eng, loci, host, dev = _pair(c, 31, generic=name == "a", **env)
    h0 = HD.start_scalars(n)
    for drv, is_host in ((host, True), (dev, False)):
        HD.configure(drv, c, moves, is_host, subst=subst, rates=rates, scalars=h0)
    hd = HD.walk(host, dev, iters, n, 1e-12 if moves == "uniform" else 1e-9, subst=subst, rates=rates, one_call=one_call,
                 exact_scalars=moves == "uniform")
    assert dev.kind() == "generic"
    assert (hd != h0).any() and (hd > 0).all()
    if name == "b":
        assert dev.streams() == 2
    dev.close(); host.close(); eng.close()


def test_state_invariants_after_a_long_run_with_heredity():
    """200 iterations on case (b)'s loci reduced to 40, the substitution moves and HRDT on: the stored density of every locus
    is the host driver's one-locus density at (tree, taus, thetas, h_i) to 1e-11 (HD.check_state; the CPU test pins that
    density to the reference's), everything else by invariants.check_state's bars — through locusrates.check_state (rates of 1):
    its P-matrix check takes the oracle at the DEVICE's category rates where alpha moves, at the same 8 ulp / 5e-16 (with the
    host routine's rates one entry of a branch of length 1.22 was 16 ulp / 7.2e-16 off here, as that module documents for
    its own run: the last places of the device's gamma quantiles, which have their own test); reading twice returns the same"""
    c = LR.case("b", 40)
    n = 40
    eng = bpp_amd.Engine(0)
    loci = tape.make_engine_loci(eng, c["data"])
    dev = bpp_amd.Sampler(eng, loci, c["data"], seed=13)
    h0 = HD.start_scalars(n)
    HD.configure(dev, c, "uniform", False, subst=True, scalars=h0)
    dev.initialize()
    HD.check_state(dev, c["data"], c["stree"][0], subst=True, loci=loci, rated=True)
    dev.iterate(200)
    seen = HD.check_state(dev, c["data"], c["stree"][0], subst=True, loci=loci, rated=True)
    print(seen)
    cnt = dev.heredity_counters()
    assert cnt[0] == 200*n and 0 < cnt[1] < cnt[0]
    h1 = dev.get_heredity()
    assert (h1 != h0).all() and (h1 > 0).all() and np.isfinite(h1).all()
    s = dev.summary()
    trees = [dev.tree(i) for i in range(n)]
    assert (dev.get_heredity() == h1).all() and dev.heredity_counters() == cnt and dev.summary() == s      # read again: nothing ran in between
    assert [dev.tree(i) for i in range(n)] == trees
    dev.close(); eng.close()


@pytest.mark.parametrize("moves", ["uniform", "program"])
def test_prior_only_run_on_the_device_leaves_every_prior(moves):
    """usedata = 0, 12 loci of the CPU twin's shape (4 species x 2 sequences: every theta can hold a coalescence; 16-lane
    groups), every move and HRDT on, 500 + 2 000 x 3 iterations: every h_i ~ gamma(4, 4), every theta and the root's tau their
    own priors — the host driver's check (tests/test_heredity_host.py), same step lengths, batch count and z bound.
    (The 32-lane form of HRDT is walked by the trajectory test's case c.  On case c's 8-species tree this run length does not
    carry the check: 15 thetas, the root's the slowest — seen there with uniform windows: every mean within 2.5 s.e., the
    root theta's sd 1.236 of the prior's against the band's 1.2 at a batch s.e. of 8 % of its mean, 7.6 s per case.)"""
    import shapes
    stree = synth.species_tree_arrays(4)
    parent, tau0, thetas = stree
    sp = [0, 0, 1, 1, 2, 2, 3, 3]
    data = shapes.shaped_set(sp, stree, [20 + k for k in range(12)], 85, model="gtr", rate_cats=4)
    eng = bpp_amd.Engine(0)
    eng.set_options(usedata=0, bfbeta=1.0)
    dev = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, data), data, seed=17)
    if moves == "program":
        dev.set_proposal_kernel(1)
        dev.set_program_moves(True, 0.3)
    dev.set_species_tree(parent, tau0, thetas)
    for i in range(12):
        dev.set_tip_species(i, sp)
    ta, tb = 6.0, 6.0/tau0[-1]
    dev.set_tau_prior(ta, tb)
    dev.set_theta_prior(4.0, 1000.0, 0.004)
    dev.set_finetune(0.008, 0.008, 0.002, 0.5)
    dev.set_heredity_move(1.5, 4.0, 4.0)
    dev.initialize()
    assert dev.kind() == "generic"
    HD.prior_marginals(dev, dev.iterate, 500, 2000, 3, 4.0, 4.0, (4.0, 1000.0), (ta, tb), [True]*len(parent))
    eng.set_options(usedata=1, bfbeta=1.0)
    dev.close(); eng.close()


def test_scalars_of_one_change_nothing_on_the_device():
    """a generic sampler with scalars explicitly 1.0 (the array exists, the kernels load from it) and the move off walks the
    trajectory of one on which nothing was set (null pointer, no load), to the bit"""
    c = LR.case("b", 40)
    eng = bpp_amd.Engine(0)
    runs = []
    for touched in (False, True):
        dev = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, c["data"]), c["data"], seed=23)
        HD.configure(dev, c, "uniform", False, subst=True, scalars=np.ones(40) if touched else None, hrdt=(0.0, 4.0, 4.0) if touched else None)
        dev.initialize()
        dev.iterate(10)
        s = dev.summary()
        runs.append(((s["total_lnl"], s["proposals"], s["accepted"]), dev.taus(), dev.thetas(), [dev.tree(i) for i in range(40)],
                     [tuple(map(tuple, map(np.atleast_1d, dev.get_subst_model(i)))) for i in range(40)]))
        assert dev.heredity_counters() == (0, 0)
        assert (dev.get_heredity() == 1.0).all()
        dev.close()
    assert runs[0] == runs[1]
    eng.close()


def test_what_the_device_samplers_refuse():
    eng = bpp_amd.Engine(0)
    parent, tau0, thetas = synth.species_tree_arrays(8)
    fit = synth.make_dataset(20, 300, 8, "jc69", 1, seed=5)
    gtr = synth.make_dataset(6, 300, 8, "gtr", 4, seed=7)

    def make(data):
        smp = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, data), data, seed=3)
        smp.set_species_tree(parent, tau0, thetas)
        smp.set_tau_prior(3.0, 3.0/tau0[-1])
        smp.set_theta_prior(2.0, 1000.0, 0.001)
        return smp
    # the persistent kernel's loci, a composite
    for data, kind in ((fit, "persistent"), (fit + gtr, "composite")):
        smp = make(data)
        with pytest.raises(bpp_amd.BpaError, match="implementation = BPA_SAMPLER_GENERIC in the options"):
            smp.set_heredity(np.full(len(data), 0.75))
        with pytest.raises(bpp_amd.BpaError, match="implementation = BPA_SAMPLER_GENERIC in the options"):
            smp.set_heredity_move(0.5, 4.0, 4.0)
        smp.set_heredity_move(0.0)                                  # nothing asked for
        assert smp.kind() == kind
        smp.close()
    # the generic sampler: bad scalars, a / b, scalars after initialize, several ranks
    smp = make(gtr)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(bpp_amd.BpaError, match="> 0 and finite"):
            smp.set_heredity([1.0, bad, 1.0, 1.0, 1.0, 1.0])
    for a, b in ((0.0, 4.0), (4.0, -1.0), (float("nan"), 4.0)):
        with pytest.raises(bpp_amd.BpaError, match="a, b > 0"):
            smp.set_heredity_move(0.5, a, b)
    with pytest.raises(bpp_amd.BpaError, match="width"):
        smp.set_heredity_move(-0.5, 4.0, 4.0)
    smp.set_heredity([1.0, 0.75, 0.25, 1.0, 0.75, 0.25])
    smp.initialize()
    assert smp.kind() == "generic"
    with pytest.raises(bpp_amd.BpaError, match="before bpa_sampler_initialize"):
        smp.set_heredity(np.ones(6))
    assert list(smp.get_heredity()) == [1.0, 0.75, 0.25, 1.0, 0.75, 0.25]
    smp.set_heredity_move(0.5, 4.0, 4.0)
    smp.iterate(1)                                                  # the supported combination runs
    assert smp.heredity_counters()[0] == 6
    before = smp.summary()["launches"]
    smp.set_allreduce(lambda p, n, st: 1, 0, 0)
    with pytest.raises(bpp_amd.BpaError, match="one rank"):
        smp.iterate(1)
    assert smp.summary()["launches"] == before                      # refused before anything was launched
    smp.close(); eng.close()
