"""Heredity scalars in the C host driver (a00_set_heredity / a00_set_heredity_move: the h_i of BPP's 'heredity = 1 a b' and
'heredity = 2 file'; gtree_update_logprob_contrib gtree.c:3859, prop_heredity gtree.c:8214) on the lnL = 0 back-end and on the
REAL reference's locus API.  GPU twin: tests/test_gpu_heredity.py; the program's posterior: tests/test_heredity_posterior.py."""
import json
import os

import numpy as np
import pytest

from bpp_amd import synth
import hostdrv
import oraclelib as O
import locusrates as LR
import heredity as HD
from common import rel

HERE = os.path.dirname(os.path.abspath(__file__))
fh = float.fromhex
needs_ref = pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref not built")


def _one_locus(case, thetas, h):
    tips = case["tips"]
    data = [dict(seqs=["A"]*tips, left=case["left"], right=case["right"], times=[fh(x) for x in case["time"]], root=case["root"])]
    drv = HD.prior_driver(data, seed=3)
    drv.set_species_tree(case["parent"], [fh(x) for x in case["tau"]], thetas)
    drv.set_tip_species(0, case["tip_species"])
    if h is not None:
        drv.set_heredity([h])
    drv.initialize()
    return drv


def test_density_is_the_references_at_theta_times_h():
    """gtree.c:3938-3943 forms heredity*theta before anything else, so the density at (theta, h) is, to the bit, the density at
    (fl(theta h), 1) — which tests/test_msc_density.py pins to gtree_logprob.  Golden trees, several sequences per species among
    them; h = 1.0 is the driver on which nothing was set, and the golden value itself"""
    cases = json.load(open(os.path.join(HERE, "golden", "msc_density.json")))
    assert len(cases) >= 19 and any(len(set(c["tip_species"])) < c["tips"] for c in cases)
    differs = 0
    for c in cases:
        theta = [fh(x) for x in c["theta"]]
        for h in (0.25, 0.75, 1.0, 3.7):
            a = _one_locus(c, theta, h)
            b = _one_locus(c, [float(np.float64(t)*np.float64(h)) for t in theta], None)
            assert a.logpr(0) == b.logpr(0) == a.tree(0)["logpr"] == b.tree(0)["logpr"], (h, a.logpr(0), b.logpr(0))
            assert a.tree(0)["pop"] == c["pop"]
            if h == 1.0:
                assert a.logpr(0) == fh(c["logpr"])
            else:
                differs += a.logpr(0) != fh(c["logpr"])
            assert list(a.get_heredity()) == [h] and list(b.get_heredity()) == [1.0]
            a.close(); b.close()
    assert differs >= 3*len(cases) - 3            # (a tree without a coalescence below the root could be indifferent)


def _several(seed, kernel, nloci=6):
    """4 species x 2 sequences, lnL = 0 -> (driver, species tree arrays)"""
    parent, tau0, thetas = synth.species_tree_arrays(4)
    sp = [0, 0, 1, 1, 2, 2, 3, 3]
    rng = np.random.default_rng(40 + seed)
    data = []
    for _ in range(nloci):
        l, r, t, rt = synth.msc_start_tree(sp, parent, tau0, thetas, rng)
        data.append(dict(seqs=["A"]*8, left=l, right=r, times=t, root=rt))
    drv = HD.prior_driver(data, seed=seed)
    if kernel:
        drv.set_proposal_kernel(1)
        drv.set_program_moves(True, 0.3)
    drv.set_species_tree(parent, tau0, thetas)
    for i in range(nloci):
        drv.set_tip_species(i, sp)
    return drv, (parent, tau0, thetas), sp


def _trajectory(drv, n, iters):
    drv.initialize()
    for _ in range(iters):
        drv.iterate()
    return (drv.counters(), drv.taus(), drv.thetas(), [drv.tree(i) for i in range(n)], [drv.logpr(i) for i in range(n)])


@pytest.mark.parametrize("kernel", [0, 1])
def test_scalars_of_one_change_nothing(kernel):
    """scalars of exactly 1.0 with the move off (its prior given, width 0): the trajectory of a driver on which nothing was
    set, to the bit, after 10 iterations of every other move"""
    runs = []
    for touched in (False, True):
        drv, (parent, tau0, thetas), _ = _several(3, kernel)
        drv.set_tau_prior(3.0, 3.0/tau0[-1]); drv.set_theta_prior(2.0, 1000.0, 0.0006); drv.set_finetune(0.003, 0.005, 0.0006, 0.2)
        if touched:
            drv.set_heredity(np.ones(6)); drv.set_heredity_move(0.0, 4.0, 4.0)
        runs.append(_trajectory(drv, 6, 10))
        assert drv.heredity_counters() == (0, 0) and (drv.get_heredity() == 1.0).all()
        drv.close()
    assert runs[0] == runs[1]
    assert runs[0][0][1] > 0


@needs_ref
def test_scalars_of_one_change_nothing_with_data():
    runs = []
    for touched in (False, True):
        data, species, (parent, tau0, thetas) = LR.mixed_host_data()
        drv = HD.reference_driver(data, seed=11)
        drv.set_species_tree(parent, tau0, thetas)
        for i, sp in enumerate(species):
            drv.set_tip_species(i, sp)
        drv.set_tau_prior(3.0, 3.0/tau0[-1]); drv.set_theta_prior(2.0, 1000.0, 0.0004)
        if touched:
            drv.set_heredity(np.ones(10)); drv.set_heredity_move(0.0)
        drv.initialize()
        for _ in range(10):
            drv.iterate()
        runs.append((drv.counters(), drv.taus(), drv.thetas(), [drv.tree(i) for i in range(10)], drv.total_lnl()))
        drv.close()
    assert runs[0] == runs[1]


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("move", [False, True])
def test_stored_densities_and_sums_follow_the_scalars(kernel, move):
    """fixed and moving scalars, every other move on, 60 iterations: every stored density is the from-scratch density at
    (tree, tau, theta, h_i) — a THETA / TAU / MIX decision or a Gibbs draw taken from sums without the 1/h_i leaves thetas whose
    stored densities still recompute, so the chain's target is checked by the prior test below; here: storage and roll-back"""
    drv, (parent, tau0, thetas), sp = _several(5, kernel)
    drv.set_tau_prior(3.0, 3.0/tau0[-1]); drv.set_theta_prior(2.0, 1000.0, 0.0006); drv.set_finetune(0.003, 0.005, 0.0006, 0.2)
    h0 = HD.start_scalars(6)
    drv.set_heredity(h0)
    if move:
        drv.set_heredity_move(0.6, 4.0, 4.0)
    drv.initialize()
    for _ in range(60):
        drv.iterate()
    h = drv.get_heredity()
    p, a = drv.heredity_counters()
    if move:
        assert p == 360 and 0 < a < p and (h != h0).any() and (h > 0).all()
    else:
        assert (p, a) == (0, 0) and (h == h0).all()
    taus, th = drv.taus(), drv.thetas()
    assert taus != list(tau0) and th != list(thetas)
    for i in range(6):
        t = drv.tree(i)
        pop, want = HD.msc_logpr(t, 8, parent, taus, th, sp, float(h[i]))
        assert pop == [int(x) for x in t["pop"]][:15]
        assert rel(t["logpr"], want) < 1e-11 and drv.logpr(i) == want, (i, t["logpr"], want)
    drv.close()


@pytest.mark.parametrize("kernel", [0, 1])
def test_prior_only_run_leaves_every_prior(kernel):
    """usedata = 0, 4 species x 2 sequences, GAGE / GSPR / THETA / TAU / MIX and HRDT on: the gene trees integrate out of
    prod_i MSC(G_i | tau, h_i theta), so every h_i comes out gamma(a, b), every theta its own gamma prior and the root's tau its
    own — a density term without h_i, a T-sum without 1/h_i in the Gibbs fits or a wrong prior ratio in HRDT shifts these
    (mean within 4.5 batch-means standard errors, sd within (0.8, 1.2) of the prior's: locusrates.gamma_check)"""
    drv, (parent, tau0, thetas), sp = _several(17 + kernel, kernel)
    ta, tb = 6.0, 6.0/tau0[-1]
    drv.set_tau_prior(ta, tb)
    drv.set_theta_prior(4.0, 1000.0, 0.004)
    drv.set_finetune(0.008, 0.008, 0.002, 0.5)
    drv.set_heredity_move(1.5, 4.0, 4.0)
    drv.initialize()

    def iterate(n):
        for _ in range(n):
            drv.iterate()
    HD.prior_marginals(drv, iterate, 1000, 4000, 3, 4.0, 4.0, (4.0, 1000.0), (ta, tb), [True]*7)
    drv.close()


def test_what_the_host_driver_refuses():
    data = synth.make_dataset(3, 60, 4, "jc69", 1, seed=3)
    drv = HD.prior_driver(data, seed=1)
    parent, tau0, thetas = synth.species_tree_arrays(4)
    drv.set_species_tree(parent, tau0, thetas)
    for bad in ([1.0, 0.0, 1.0], [1.0, -2.0, 1.0], [1.0, float("nan"), 1.0], [float("inf"), 1.0, 1.0]):
        assert not drv.try_set_heredity(bad)
    assert (drv.get_heredity() == 1.0).all()                             # a refused call leaves nothing behind
    for a, b in ((0.0, 4.0), (4.0, 0.0), (-1.0, 4.0), (4.0, float("nan")), (float("inf"), 4.0)):
        assert not drv.try_set_heredity_move(0.5, a, b)
    assert drv.try_set_heredity_move(0.0, 0.0, 0.0)                      # the move off: a, b are not used
    assert not drv.try_set_heredity_move(-0.5, 4.0, 4.0) and not drv.try_set_heredity_move(float("nan"), 4.0, 4.0)
    assert drv.try_set_heredity([0.25, 0.75, 1.0])
    drv.initialize()
    assert not drv.try_set_heredity([1.0, 1.0, 1.0])                     # the start-up densities have used them
    assert list(drv.get_heredity()) == [0.25, 0.75, 1.0]
    assert drv.try_set_heredity_move(0.5, 4.0, 4.0)                      # the move goes on in mid-run
    drv.iterate()
    assert drv.heredity_counters()[0] == 3
    drv.close()
