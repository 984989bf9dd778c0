"""Per-locus mutation rates in the C host driver (a00_set_locus_rates / a00_set_locusrate_moves: BPP's mu_i and mu_bar
moves under the conditional-iid prior, stree.c:9225 / 9770) on the REAL reference's locus API and on the lnL = 0 back-end.
GPU twin: tests/test_gpu_locusrates.py."""
import numpy as np
import pytest

from bpp_amd import synth
import oraclelib as O
import locusrates as LR
from common import rel

needs_ref = pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref not built")


def _mixed(seed, rates=None):
    data, species, (parent, tau0, thetas) = LR.mixed_host_data()
    drv = LR.reference_driver(data, seed=seed)
    drv.set_species_tree(parent, tau0, thetas)
    for i, sp in enumerate(species):
        drv.set_tip_species(i, sp)
    drv.set_tau_prior(3.0, 3.0/tau0[-1])
    drv.set_theta_prior(2.0, 1000.0, 0.0004)
    if rates is not None:
        drv.set_locus_rates(rates)
    return drv, data, species, parent


@needs_ref
def test_fixed_rates_scale_every_branch_length():
    """rates 0.25 .. 4, moves off: the start-up likelihood of every locus is the oracle's at lengths x mu_i (the project's
    1e-13 bar), and after 20 iterations of all other moves the rates are what they were and every held quantity is still its
    recompute (a length left unscaled by some move fails here)"""
    rates = LR.spread_rates(10, 0.25, 4.0)
    drv, data, species, parent = _mixed(7, rates)
    drv.initialize()
    for i, d in enumerate(data):
        t = drv.tree(i)
        assert rel(t["lnl"], LR.oracle_lnl(d, t, rates[i])) < 1e-13, i
        assert t["lnl"] != LR.oracle_lnl(d, t, 1.0)
    for _ in range(20):
        drv.iterate()
    got, mubar = drv.get_locus_rates()
    assert (got == rates).all() and mubar == 1.0
    assert drv.locusrate_counters() == dict(mui=(0, 0), mubar=(0, 0))
    LR.check_state(drv, data, parent, tip_species=species)
    p, a, _ = drv.counters()
    assert 0.05 < a/p < 0.98
    drv.close()


@needs_ref
def test_rates_of_one_change_nothing():
    """x*1.0 == x: a driver given rates of 1.0 (and the moves' parameters, widths 0) walks the trajectory of one on which the
    new calls were never made — ages, trees, likelihoods to the bit"""
    runs = []
    for touched in (False, True):
        drv, data, species, parent = _mixed(11, np.ones(10) if touched else None)
        if touched:
            drv.set_locusrate_moves(0.0, 0.0, 5.0, 10.0, 10.0, 1.0)
        drv.initialize()
        for _ in range(10):
            drv.iterate()
        runs.append((drv.counters(), drv.taus(), drv.thetas(), [drv.tree(i) for i in range(len(data))], drv.total_lnl()))
        drv.close()
    a, b = runs
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and a[4] == b[4]
    for x, y in zip(a[3], b[3]):
        assert x == y


@needs_ref
def test_moves_keep_the_state_invariants_with_cohorts_and_threads():
    """MUI + MUBAR on (both proposal kernels): the rates move, every held likelihood is the oracle's at the CURRENT rate, and
    two cohorts / three threads walk the same trajectory"""
    for kernel in (0, 1):
        runs = []
        for cohorts in (False, True):
            data, species, (parent, tau0, thetas) = LR.mixed_host_data()
            import hostdrv
            drv = LR.RateDriver(hostdrv.reference_driver_cohorts(data, 4, seed=5) if cohorts else hostdrv.reference_driver(data, seed=5))
            drv.set_threads(3 if cohorts else 1)
            drv.set_proposal_kernel(kernel)
            if kernel:
                drv.set_program_moves(True, 0.3)
            drv.set_species_tree(parent, tau0, thetas)
            for i, sp in enumerate(species):
                drv.set_tip_species(i, sp)
            drv.set_tau_prior(3.0, 3.0/tau0[-1])
            drv.set_theta_prior(2.0, 1000.0, 0.0004)
            drv.set_locus_rates(LR.spread_rates(10, 0.5, 2.0))
            drv.set_locusrate_moves(0.5, 0.4, 5.0, 10.0, 10.0, 1.0)
            drv.initialize()
            for _ in range(12):
                drv.iterate()
            r, m = drv.get_locus_rates()
            c = drv.locusrate_counters()
            assert c["mui"][0] == 120 and 0 < c["mui"][1] < 120 and c["mubar"][0] == 12 and 0 < c["mubar"][1]
            assert m != 1.0 and (r != LR.spread_rates(10, 0.5, 2.0)).any()
            LR.check_state(drv, data, parent, tip_species=species)
            runs.append((drv.counters()[:2], list(r), m, [drv.tree(i) for i in range(len(data))], drv.total_lnl()))
            drv.close()
        assert runs[0] == runs[1], kernel


@pytest.mark.parametrize("mubar_prior", [(10.0, 10.0), None])
def test_prior_only_run_leaves_the_priors_of_the_rates(mubar_prior):
    """lnL = 0 with MUI and MUBAR on: the joint of the rates is p(mu_bar) prod_i gamma(mu_i | a_mui, a_mui/mu_bar), so the
    marginal of mu_bar is its gamma(10, 10) prior and that of every mu_i / mu_bar is gamma(5, 5), exactly — a wrong Jacobian or
    prior term in either move shifts these means.  mu_bar fixed (a_mubar = b_mubar = 0): no MUBAR step runs, mu_i ~ gamma(5, 5)"""
    data = synth.make_dataset(12, 60, 4, "jc69", 1, seed=3)
    drv = LR.prior_driver(data, seed=17)
    parent, tau0, thetas = synth.species_tree_arrays(4)
    drv.set_species_tree(parent, tau0, thetas)
    a, b = mubar_prior if mubar_prior else (0.0, 0.0)
    drv.set_locusrate_moves(1.2, 0.6, 5.0, a, b, 1.0)
    drv.initialize()

    def iterate(n):
        for _ in range(n):
            drv.iterate()
    LR.prior_marginals(drv, iterate, 1000, 4000, 3, 5.0, mubar_prior)
    drv.close()


def test_what_the_host_driver_refuses():
    data = synth.make_dataset(3, 60, 4, "jc69", 1, seed=3)
    drv = LR.prior_driver(data, seed=1)
    parent, tau0, thetas = synth.species_tree_arrays(4)
    drv.set_species_tree(parent, tau0, thetas)
    for bad in ([1.0, 0.0, 1.0], [1.0, -2.0, 1.0], [1.0, float("nan"), 1.0], [float("inf"), 1.0, 1.0]):
        assert not drv.try_set_locus_rates(bad)
    assert (drv.get_locus_rates()[0] == 1.0).all()                       # a refused call leaves nothing behind
    for a_mui in (0.0, -1.0, float("nan")):
        assert not drv.try_set_locusrate_moves(0.5, 0.0, a_mui)
        assert not drv.try_set_locusrate_moves(0.0, 0.5, a_mui, 10.0, 10.0)
    assert drv.try_set_locusrate_moves(0.0, 0.0, 0.0)                    # both moves off: a_mui is not used
    assert not drv.try_set_locusrate_moves(-0.5, 0.0, 5.0)
    assert drv.try_set_locus_rates([0.5, 1.0, 2.0])
    drv.initialize()
    assert not drv.try_set_locus_rates([1.0, 1.0, 1.0])                  # the start-up evaluation has used them
    assert list(drv.get_locus_rates()[0]) == [0.5, 1.0, 2.0]
    assert drv.try_set_locusrate_moves(0.5, 0.5, 5.0, 10.0, 10.0, 0.0)   # widths change in mid-run; mubar 0: keep the current one
    assert drv.get_locus_rates()[1] == 1.0
    drv.close()
