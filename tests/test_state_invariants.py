"""tests/invariants.py: check_state on the C host driver over the REAL reference's locus API (hostdrv.reference_driver)
after hundreds of iterations — every held quantity equals its from-scratch recompute — and, the other half, on states with
one thing wrong at a time: the checker must fail on each.  GPU twin: tests/test_gpu_state_invariants.py."""
import copy

import numpy as np
import pytest

from bpp_amd import synth
import oraclelib as O
import hostdrv
from invariants import check_state, several_sequences_data, moved

pytestmark = pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref not built")


def run(data, taxa, iters, moves, seed=7, scaling=False, subst=False, species=None, stree=None, checks=()):
    drv = hostdrv.reference_driver(data, seed=seed, scaling=scaling)
    parent, tau0, thetas = stree or synth.species_tree_arrays(taxa)
    if moves == "program":
        drv.set_proposal_kernel(1)
        drv.set_program_moves(True, 0.3)
    drv.set_species_tree(parent, tau0, thetas)
    if species is not None:
        for i in range(len(data)):
            drv.set_tip_species(i, species)
    drv.set_tau_prior(3.0, 3.0 / tau0[-1])
    drv.set_theta_prior(2.0, 1000.0, 0.0004)
    drv.set_finetune(0.003, 0.005, 0.0004, 0.05)
    R = data[0]["rate_cats"]
    if subst:
        drv.set_subst_moves(0.3, 0.4, 0.8, 1.0, 1.0)
        for i, d in enumerate(data):
            drv.set_subst_model(i, list(d["freqs"]), list(d["exch"]), 0.5, R)
    drv.initialize()
    kw = dict(tip_species=None if species is None else [species] * len(data), scaling=scaling, subst=subst or None)
    check_state(drv, data, parent, **kw)
    for it in range(1, iters + 1):
        drv.iterate()
        if it in checks:
            check_state(drv, data, parent, **kw)
    seen = check_state(drv, data, parent, **kw)
    p, a, _ = drv.counters()
    moved(drv, tau0, thetas, p, a)
    return drv, seen, (parent, tau0, thetas)


@pytest.mark.parametrize("taxa,nloci,iters,moves", [(4, 200, 300, "program"), (8, 60, 150, "program"), (8, 60, 150, "uniform"), (6, 60, 150, "uniform")])
def test_held_state_equals_recompute_after_a_long_run(taxa, nloci, iters, moves):
    data = synth.make_dataset(nloci, 300, taxa, "jc69", 1, seed=17)
    drv, seen, _ = run(data, taxa, iters, moves, checks=(1, 10, 100))
    assert seen["lnl"] < 1e-12 and seen["logpr"] < 1e-11
    drv.close()


def test_held_state_with_parameter_moves():
    """GTR + Gamma4 with the frequency / exchangeability / alpha moves on: the oracle takes each locus's CURRENT parameters"""
    data = synth.make_dataset(40, 300, 8, "gtr", 4, seed=23)
    drv, seen, _ = run(data, 8, 150, "program", subst=True, checks=(3, 30))
    assert any(drv.get_subst_model(i)[2] != 0.5 for i in range(len(data)))
    drv.close()


@pytest.mark.parametrize("moves", ["uniform", "program"])
def test_held_state_with_several_sequences_per_species(moves):
    """tip populations hold coalescences, gene nodes cross the species boundary both ways"""
    data, species, stree = several_sequences_data()
    drv, seen, _ = run(data, None, 200, moves, species=species, stree=stree, checks=(8,))
    assert sum(sum(int(x) == 2 for x in drv.tree(i)["pop"][6:]) != 1 for i in range(len(data))) > 0
    drv.close()


@pytest.mark.parametrize("taxa,model,R", [(6, "jc69", 2), (8, "gtr", 4)])
def test_held_state_with_scale_buffers(taxa, model, R):
    data = synth.make_dataset(20, 300, taxa, model, R, seed=31)
    drv, seen, _ = run(data, taxa, 100, "uniform", scaling=True, checks=(2,))
    drv.close()


# ------------------------------------------------------------------ the checker fails when it should
class Frozen:
    """a state taken out of a driver, with the driver's interface: one thing at a time is then changed in it"""

    def __init__(self, drv, n):
        self.trees = [copy.deepcopy(drv.tree(i)) for i in range(n)]
        self._taus, self._thetas, self._total = list(drv.taus()), list(drv.thetas()), drv.total_lnl()

    def tree(self, i):
        return self.trees[i]

    def taus(self):
        return list(self._taus)

    def thetas(self):
        return list(self._thetas)

    def total_lnl(self):
        return self._total


@pytest.fixture(scope="module")
def state():
    taxa, nloci = 8, 40
    data = synth.make_dataset(nloci, 300, taxa, "jc69", 1, seed=41)
    drv = hostdrv.reference_driver(data, seed=13)
    parent, tau0, thetas = synth.species_tree_arrays(taxa)
    drv.set_proposal_kernel(1)
    drv.set_program_moves(True, 0.3)
    drv.set_species_tree(parent, tau0, thetas)
    drv.set_tau_prior(3.0, 3.0 / tau0[-1])
    drv.set_theta_prior(2.0, 1000.0, 0.0004)
    drv.set_finetune(0.003, 0.005, 0.0004, 0.05)
    drv.initialize()
    before = None
    for it in range(60):
        before = [drv.tree(i)["lnl"] for i in range(nloci)]
        drv.iterate()
    frozen = Frozen(drv, nloci)
    drv.close()
    return data, parent, frozen, before


def test_the_frozen_state_passes(state):
    data, parent, frozen, _ = state
    seen = check_state(frozen, data, parent)
    assert seen["lnl"] < 1e-12


def _inner_non_root(t, tips):
    return next(v for v in range(tips, 2 * tips - 1) if v != t["root"])


def test_checker_sees_an_inner_age_off_by_one_part_in_a_million(state):
    data, parent, frozen, _ = state
    f = copy.deepcopy(frozen)
    v = _inner_non_root(f.trees[5], 8)
    f.trees[5]["time"][v] *= 1 + 1e-6
    with pytest.raises(AssertionError, match=r"locus 5 (logpr|lnl)"):
        check_state(f, data, parent)


def test_checker_sees_a_root_age_off_by_one_part_in_a_million(state):
    """(the root's age enters the likelihood through two branches only)"""
    data, parent, frozen, _ = state
    f = copy.deepcopy(frozen)
    f.trees[9]["time"][f.trees[9]["root"]] *= 1 + 1e-6
    with pytest.raises(AssertionError, match=r"locus 9 (logpr|lnl)"):
        check_state(f, data, parent)


def test_checker_sees_a_likelihood_from_before_the_last_accepted_move(state):
    data, parent, frozen, before = state
    f = copy.deepcopy(frozen)
    i = next(k for k in range(len(data)) if before[k] != f.trees[k]["lnl"])      # a locus whose last iteration accepted a move
    f.trees[i]["lnl"] = before[i]
    with pytest.raises(AssertionError, match=rf"locus {i} lnl"):
        check_state(f, data, parent)


def test_checker_sees_a_stale_total(state):
    data, parent, frozen, before = state
    f = copy.deepcopy(frozen)
    i = next(k for k in range(len(data)) if before[k] != f.trees[k]["lnl"])
    f._total += before[i] - f.trees[i]["lnl"]
    with pytest.raises(AssertionError, match="total lnl"):
        check_state(f, data, parent)


def test_checker_sees_a_population_label_one_too_high(state):
    data, parent, frozen, _ = state
    f = copy.deepcopy(frozen)
    i, v = next((i, v) for i in range(len(data)) for v in range(8, 15) if parent[f.trees[i]["pop"][v]] >= 0)
    f.trees[i]["pop"][v] = parent[f.trees[i]["pop"][v]]
    with pytest.raises(AssertionError, match=rf"locus {i} node {v}: age .* below its population"):
        check_state(f, data, parent)


def test_checker_sees_a_tip_in_another_species(state):
    """a tip's label is bound by no age (its age is 0 in every tip population): it is compared with the tip's species"""
    data, parent, frozen, _ = state
    f = copy.deepcopy(frozen)
    f.trees[3]["pop"][0] = 1
    with pytest.raises(AssertionError, match=r"locus 3 node 0: tip population"):
        check_state(f, data, parent)


def test_checker_sees_a_theta_changed_after_the_fact(state):
    data, parent, frozen, _ = state
    f = copy.deepcopy(frozen)
    f._thetas[-1] *= 1.0001                        # the root population's: every locus's logpr is stale
    with pytest.raises(AssertionError, match=r"locus 0 logpr"):
        check_state(f, data, parent)


def test_checker_sees_a_tau_changed_after_the_fact(state):
    data, parent, frozen, _ = state
    f = copy.deepcopy(frozen)
    f._taus[-1] *= 1 + 1e-9                        # (no age bound is crossed by so little: the density is what is stale)
    with pytest.raises(AssertionError, match=r"logpr|below its population|beyond the end"):
        check_state(f, data, parent)


def test_checker_sees_two_inner_nodes_on_one_clv_buffer(state):
    data, parent, frozen, _ = state
    f = copy.deepcopy(frozen)
    f.trees[7]["clv"][9] = f.trees[7]["clv"][8]
    with pytest.raises(AssertionError, match=r"locus 7: two inner nodes share a CLV index"):
        check_state(f, data, parent)


def test_checker_sees_two_nodes_on_one_pmatrix(state):
    data, parent, frozen, _ = state
    f = copy.deepcopy(frozen)
    t = f.trees[7]
    a, b = [v for v in range(15) if v != t["root"]][:2]
    t["pmat"][a] = t["pmat"][b]
    with pytest.raises(AssertionError, match=r"locus 7: two nodes share a P-matrix index"):
        check_state(f, data, parent)


def test_checker_sees_a_child_older_than_its_parent(state):
    data, parent, frozen, _ = state
    f = copy.deepcopy(frozen)
    t = f.trees[11]
    v = _inner_non_root(t, 8)
    t["time"][v] = t["time"][t["parent"][v]] * 1.01
    with pytest.raises(AssertionError, match=rf"locus 11 node {v}: age .* not below its parent"):
        check_state(f, data, parent)


def test_checker_sees_a_parent_link_that_is_not_the_inverse_of_the_child_links(state):
    data, parent, frozen, _ = state
    f = copy.deepcopy(frozen)
    t = f.trees[2]
    v = _inner_non_root(t, 8)
    t["parent"][v] = next(u for u in range(8, 15) if u not in (v, t["parent"][v]))
    with pytest.raises(AssertionError, match=rf"locus 2 node {v}: parent"):
        check_state(f, data, parent)
