"""Per-locus mutation rates on the generic device sampler (bpa_sampler_set_locus_rates / bpa_sampler_set_locusrate_moves:
BPP's mu_i and mu_bar moves, stree.c:9225 / 9770 — step mode 9 of gsm::gstep_kernel, gsm::gmubar_kernel) against the C host
driver on the same library, against a CPU recompute, against the priors, and what the other samplers refuse.
CPU twin: tests/test_locusrates_host.py."""
import numpy as np
import pytest

import bpp_amd
from bpp_amd import synth
import tape
import locusrates as LR
import shapes

pytestmark = pytest.mark.gpu


def _pair(c, seed, generic=False, **options):
    """(engine, engine loci of the device sampler, host driver, device sampler) on case c's data"""
    eng = bpp_amd.Engine(0)
    data = c["data"]
    loci_a = tape.make_engine_loci(eng, data)
    loci_b = tape.make_engine_loci(eng, data)
    host = LR.hip_driver(eng, loci_a, data, seed=seed)
    dev = bpp_amd.Sampler(eng, loci_b, data, seed=seed, implementation="generic" if generic else None, **options)
    return eng, loci_b, host, dev


# case, moves, iterations, options, mu_bar prior (None: fixed), what must hold besides the trajectory
TRAJECTORIES = [
    ("a", "uniform", 5, None, (10.0, 10.0)),                       # 70 loci: two workgroups of gstep_kernel; the chain launch
    ("a", "uniform", 5, dict(chain=False), (10.0, 10.0)),           # ... and a launch per step
    ("a", "program", 3, None, (10.0, 10.0)),                       # BPP's kernel, MUBAR decided on the device from GDecState::z
    ("a", "program", 3, dict(host_decisions=True), (10.0, 10.0)),         # ... and on the host
    ("b", "uniform", 5, None, (10.0, 10.0)),                       # two part-batches, fuse_pm, MUI after the alpha step
    ("b", "program", 3, None, (10.0, 10.0)),
    ("b", "program", 3, dict(host_decisions=True), (10.0, 10.0)),
    ("c", "uniform", 5, None, None),                               # 16 tips: 32-lane groups; mu_bar fixed
    ("d", "uniform", 5, None, (10.0, 10.0)),                       # 20-state records, parts of the loci
    # mu_bar fixed and ALL iterations in one call: the rate step that ends an iteration is settled inside the next iteration's
    # first proposal launch (LR.walk: one_call) — the lane groups' settle of mode 9, 16 and 32 lanes, fuse_pm on, both
    # proposal kernels, the 20-state records
    ("b", "uniform", 5, dict(one_call=True), None),
    ("b", "program", 3, dict(one_call=True), None),
    ("c", "uniform", 5, dict(one_call=True), None),
    ("d", "uniform", 5, dict(one_call=True), None),
    ("a", "uniform", 5, dict(one_call=True, chain=False), None),
]


@pytest.mark.parametrize("name,moves,iters,env,mubar_prior", TRAJECTORIES, ids=shapes.option_id)
def test_device_sampler_with_rate_moves_equals_host_driver(name, moves, iters, env, mubar_prior):
    """rates spread over 0.5 .. 2, MUI + MUBAR on: same decisions, counters, trees and buffer indices as the host driver's
    mui_step / mubar_step; ages, taus, thetas to walk's tolerances (1e-12 uniform, 1e-9 with the program's moves: libm on both
    sides of a Bactrian-Laplace window), rates and their mean to 1e-11 (exp / log of device libm against glibc: the
    substitution parameters' bar), total lnL to 1e-10"""
    c = LR.case(name)
    n = len(c["data"])
    subst = name == "b"
    env = dict(env or {})
    one_call = env.pop("one_call", False)
    eng, loci, host, dev = _pair(c, 29, generic=name == "a", **env)
    rates = LR.spread_rates(n, 0.5, 2.0)
    for drv, is_host in ((host, True), (dev, False)):
        LR.configure(drv, c, moves, is_host, subst=subst, mubar_prior=mubar_prior, rates=rates)
    rd, md = LR.walk(host, dev, iters, n, 1e-12 if moves == "uniform" else 1e-9, subst=subst, one_call=one_call)
    assert dev.kind() == "generic"
    cnt = dev.locusrate_counters()
    assert cnt["mui"][0] == iters*n and 0 < cnt["mui"][1] < iters*n
    assert (rd != rates).any()
    if mubar_prior is None:
        assert cnt["mubar"] == (0, 0) and md == 1.0
    else:
        assert cnt["mubar"][0] == iters
    if name in ("b", "d"):
        assert dev.streams() == 2
    # the downloaded likelihoods are the oracle's at lengths x mu_i
    for i in range(0, n, max(1, n//6)):
        t = dev.tree(i)
        par = dev.get_subst_model(i) if subst else None
        assert LR.rel(t["lnl"], LR.oracle_lnl(c["data"][i], t, rd[i], par)) < 1e-10, i
    dev.close(); host.close(); eng.close()


@pytest.mark.parametrize("mubar_prior", [(10.0, 10.0), None])
def test_state_invariants_after_a_long_run_with_rate_moves(mubar_prior):
    """200 iterations on case (b)'s loci reduced to 40, the substitution moves and the rate moves on: everything the sampler
    holds per locus is its CPU recompute from (tree, taus, thetas, substitution parameters, mu_i) — lnl and the root buffer to
    1e-10, logpr to 1e-11, every inner CLV the node update of its children's buffers, every P-matrix buffer within the
    project's bar of the oracle's at (t_parent - t_child) mu_i.  mu_bar fixed: every MUI step of the 200 is settled inside the
    next iteration's first proposal launch, whose lane groups then fill the P-matrices at the settled rate.
    P-matrices (LR.check_buffers): 8 ulp or 5e-16 (the project's bar, invariants.check_state's), against the eigen form
    of the device's OWN eigensystem and category rates at the scaled length, and against the oracle's from the locus's
    parameters with the device's category rates.  These loci's trees grow long (scaled lengths of order 1); with the HOST
    routine's category rates in the oracle one entry was 10 ulp / 5.55e-16 (first seen as 21 ulp / 5.55e-16) from the oracle's
    while the own-eigensystem form held: the last places of the device's gamma quantiles, which have their own test."""
    c = LR.case("b", 40)
    n = 40
    eng = bpp_amd.Engine(0)
    loci = tape.make_engine_loci(eng, c["data"])
    dev = bpp_amd.Sampler(eng, loci, c["data"], seed=13)
    rates = LR.spread_rates(n, 0.5, 2.0)
    LR.configure(dev, c, "uniform", False, subst=True, rates=rates, mubar_prior=mubar_prior)
    dev.initialize()
    LR.check_state(dev, c["data"], c["stree"][0], subst=True, loci=loci)
    dev.iterate(200)
    seen = LR.check_state(dev, c["data"], c["stree"][0], subst=True, loci=loci)
    print(seen)
    cnt = dev.locusrate_counters()
    assert cnt["mui"][0] == 200*n and 0 < cnt["mui"][1] < cnt["mui"][0]
    if mubar_prior is None:
        assert cnt["mubar"] == (0, 0)
    else:
        assert cnt["mubar"][0] == 200 and 0 < cnt["mubar"][1] < 200
    r1, m1 = dev.get_locus_rates()
    assert (r1 != rates).all() and (m1 != 1.0) == (mubar_prior is not None) and (r1 > 0).all() and np.isfinite(r1).all()
    s = dev.summary()
    r2, m2 = dev.get_locus_rates()                                   # read again: nothing ran in between
    assert (r1 == r2).all() and m1 == m2 and dev.locusrate_counters() == cnt and dev.summary() == s
    dev.close(); eng.close()


@pytest.mark.parametrize("mubar_prior", [(10.0, 10.0), None])
def test_prior_only_run_on_the_device_leaves_the_priors_of_the_rates(mubar_prior):
    """usedata = 0: mu_bar ~ gamma(10, 10) and every mu_i / mu_bar ~ gamma(5, 5) (mu_bar fixed: mu_i ~ gamma(5, 5), no MUBAR
    step) — the host driver's check (tests/test_locusrates_host.py) with mode 9's prior and Jacobian terms and gmubar_kernel's
    decision in it, same batch count and z bound"""
    c = LR.case("b", 12)
    eng = bpp_amd.Engine(0)
    eng.set_options(usedata=0, bfbeta=1.0)
    dev = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, c["data"]), c["data"], seed=17)
    LR.configure(dev, c, "uniform", False, ft=(1.2, 0.6), mubar_prior=mubar_prior)
    dev.initialize()
    assert dev.kind() == "generic"
    LR.prior_marginals(dev, dev.iterate, 500, 2000, 3, 5.0, mubar_prior)
    eng.set_options(usedata=1, bfbeta=1.0)
    dev.close(); eng.close()


def test_rates_of_one_change_nothing_on_the_device():
    """x*1.0 == x: a generic sampler with rates explicitly 1.0 (the rate arrays exist, the kernels load from them) and the moves
    off walks the trajectory of one on which nothing was set (null pointers, no load), to the bit"""
    c = LR.case("b", 40)
    eng = bpp_amd.Engine(0)
    runs = []
    for touched in (False, True):
        dev = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, c["data"]), c["data"], seed=23)
        LR.configure(dev, c, "uniform", False, subst=True, ft=None, rates=np.ones(40) if touched else None)
        if touched:
            dev.set_locusrate_moves(0.0, 0.0, 5.0, 10.0, 10.0, 1.0)
        dev.initialize()
        dev.iterate(10)
        s = dev.summary()
        runs.append(((s["total_lnl"], s["proposals"], s["accepted"]), dev.taus(), dev.thetas(), [dev.tree(i) for i in range(40)],
                     [tuple(map(tuple, map(np.atleast_1d, dev.get_subst_model(i)))) for i in range(40)]))
        assert dev.locusrate_counters() == dict(mui=(0, 0), mubar=(0, 0))
        assert (dev.get_locus_rates()[0] == 1.0).all()
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
            smp.set_locus_rates(np.full(len(data), 1.5))
        with pytest.raises(bpp_amd.BpaError, match="implementation = BPA_SAMPLER_GENERIC in the options"):
            smp.set_locusrate_moves(0.5, 0.0, 5.0)
        smp.set_locusrate_moves(0.0, 0.0, 0.0)                      # nothing asked for
        assert smp.kind() == kind
        smp.close()
    # the generic sampler: bad rates, a_mui, rates after initialize, several ranks
    smp = make(gtr)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(bpp_amd.BpaError, match="> 0 and finite"):
            smp.set_locus_rates([1.0, bad, 1.0, 1.0, 1.0, 1.0])
    with pytest.raises(bpp_amd.BpaError, match="a_mui"):
        smp.set_locusrate_moves(0.5, 0.0, 0.0)
    with pytest.raises(bpp_amd.BpaError, match="a_mui"):
        smp.set_locusrate_moves(0.0, 0.5, -1.0, 10.0, 10.0)
    smp.set_locus_rates([0.5, 0.8, 1.0, 1.2, 1.5, 2.0])
    smp.initialize()
    assert smp.kind() == "generic"
    with pytest.raises(bpp_amd.BpaError, match="before bpa_sampler_initialize"):
        smp.set_locus_rates(np.ones(6))
    assert list(smp.get_locus_rates()[0]) == [0.5, 0.8, 1.0, 1.2, 1.5, 2.0]
    smp.set_locusrate_moves(0.5, 0.4, 5.0, 10.0, 10.0, 1.0)
    smp.iterate(1)                                                  # the supported combination runs
    before = smp.summary()["launches"]
    smp.set_allreduce(lambda p, n, st: 1, 0, 0)
    with pytest.raises(bpp_amd.BpaError, match="one rank"):
        smp.iterate(1)
    assert smp.summary()["launches"] == before                      # refused before anything was launched
    smp.close(); eng.close()
