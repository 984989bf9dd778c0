"""Per-locus mutation rates and heredity scalars on the big-tree device sampler (csrc/bigsampler.hpp: the h of tree_logpr, the
lengths x mu_i of the record loop, step modes 9 — MUI, settled as pend 4 — and 10 — HRDT — of big_step_kernel, both
instantiations; csrc/gsampler_host.hpp: gs_iterate's tail / gs_mubar) against the C host driver on the same library, against the
oracle's scale counters at lengths x mu_i, against a CPU recompute, against the priors, and what stays refused.
CPU twin: tests/test_bigsampler_scalars_host.py; the generic sampler's tests: tests/test_gpu_heredity.py, tests/test_gpu_locusrates.py."""
import json
import os

import numpy as np
import pytest

import bpp_amd
from bpp_amd import synth, seqio
import firing
import heredity as HD
import hostdrv
import invariants
import locusrates as LR
import oraclelib as O
import shapes
import tape
from common import rel

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HRDT = (0.6, 4.0, 4.0)                       # heredity.configure's width and gamma(a, b)
RATE_FT, A_MUI, MUBAR_PRIOR = (0.5, 0.4), 5.0, (10.0, 10.0)      # ... and its rate moves (locusrates.configure's defaults)


# ------------------------------------------------------------------ 1. the host driver's trajectory
def _frogs():
    """the loci, start trees, species tree, priors and step lengths of
    tests/test_gpu_bigsampler_program.py::test_big_sampler_program_moves_on_the_frogs_loci -> (case dict, engine-locus maker)"""
    from test_gpu_host_driver import _msc_start_tree
    gold = json.load(open(os.path.join(G, "input_pipeline.json")))
    recs = seqio.load_dataset(os.path.join(G, "frogs", "frogs.txt"), os.path.join(G, "frogs", "frogs.Imap.txt"), gold["species"], [1, 1, 1, 1], model="jc69")
    parent = [4, 4, 5, 6, 5, 6, -1]                       # K C L H | KC KCL root
    tau0 = [0.0] * 4 + [0.01, 0.02, 0.03]
    thetas = [0.02] * 7
    rng = np.random.default_rng(9)
    data = []
    for r in recs:
        left, right, times, root = _msc_start_tree(r["species"], parent, tau0, thetas, rng)
        data.append(dict(seqs=r["seqs"], weights=r.get("weights", np.ones(len(r["seqs"][0]))), left=left, right=right, times=times, root=root,
                         states=4, rate_cats=1, model="jc69", rates=np.ones(1)))
    assert max(len(r["seqs"]) for r in recs) > 16
    c = dict(data=data, species=[r["species"] for r in recs], stree=(parent, tau0, thetas), model="jc69", scaling=False)
    return c, lambda eng: [seqio.make_locus(eng, r) for r in recs]


def _trajectory_case(name):
    """-> (case dict with `model` and `scaling`, engine-locus maker or None: tape.make_engine_loci, forced onto the sampler)"""
    if name in ("big-17-30", "big-64-30"):
        return dict(shapes.case(name), model="jc69", scaling=name == "big-64-30"), None, False
    if name == "forced-4-jc":
        # 40 loci: more than one wave of the sum kernels' workgroup holds, fewer than its 1 024 lanes
        return dict(data=synth.make_dataset(40, 300, 4, "jc69", 1, seed=19), species=None, stree=synth.species_tree_arrays(4), model="jc69", scaling=False), None, True
    if name == "forced-8-gtr":
        return dict(LR.case("b", 12), scaling=False), None, True
    assert name == "frogs"
    c, make = _frogs()
    return c, make, False


def _configure(drv, c, moves, host, ft, frogs):
    """species tree, priors, step lengths and move set (locusrates.configure's; the frogs: their own test's), then rates on
    (0.5, 2) with MUI (and MUBAR where ft[1] > 0) and scalars on (0.25, 2) with HRDT — the same calls on both sides"""
    n = len(c["data"])
    rates, h0 = LR.spread_rates(n, 0.5, 2.0), HD.start_scalars(n)
    if not frogs:
        LR.configure(drv, c, moves, host, ft=ft, a_mui=A_MUI, mubar_prior=MUBAR_PRIOR, rates=rates)
    else:
        parent, tau0, thetas = c["stree"]
        drv.set_proposal_kernel(1)
        drv.set_program_moves(True, 0.3)
        drv.set_species_tree(parent, tau0, thetas)
        for i, sp in enumerate(c["species"]):
            drv.set_tip_species(i, sp)
        drv.set_tau_prior(3.0, 100.0)
        drv.set_theta_prior(3.0, 150.0, 0.003)
        drv.set_finetune(0.004, 0.004, 0.002, 0.1)
        drv.set_locus_rates(rates)
        drv.set_locusrate_moves(ft[0], ft[1], A_MUI, MUBAR_PRIOR[0], MUBAR_PRIOR[1], 1.0)
    drv.set_heredity(h0)
    drv.set_heredity_move(*HRDT)
    return rates, h0


# case, moves, iterations, all iterations in one call with the mu_bar move off
TRAJECTORIES = [
    ("big-17-30", "uniform", 3, False),
    ("big-17-30", "program", 3, False),
    ("big-64-30", "program", 2, False),                    # scale buffers
    ("forced-4-jc", "uniform", 5, False),                  # many loci: the uniform sum kernels divide by h_i over several waves
    ("forced-4-jc", "program", 5, False),                  # ... and the program's (gdec_theta_sums_kernel, gdec_sums_kernel)
    ("forced-8-gtr", "program", 3, False),                 # GTR + Gamma4: P-matrices from the eigen form at lengths x mu_i
    ("frogs", "program", 2, False),                        # unphased diploids of 42-60 tips
    ("big-17-30", "uniform", 3, True),                     # MUI closes the iteration: settled inside the next one's first launch
    ("big-17-30", "program", 3, True),
]


@pytest.mark.parametrize("name,moves,iters,one_call", TRAJECTORIES)
def test_big_tree_sampler_with_scalars_equals_host_driver(name, moves, iters, one_call):
    """rates log-uniform on (0.5, 2), scalars on (0.25, 2), HRDT + MUI + MUBAR on together (one_call: MUBAR off): the decisions,
    both counter families, trees, populations and buffer indices of the host driver's hered_step / mui_step / mubar_step in
    a00_iterate's order, through heredity.walk at its own bars — ages, taus, thetas 1e-12 with uniform windows (scalars ==),
    1e-9 with the program's moves; logpr 1e-11, lnL 1e-10, rates and their mean 1e-11"""
    c, make, forced = _trajectory_case(name)
    data = c["data"]
    n = len(data)
    eng = bpp_amd.Engine(0)
    loci_of = make or (lambda e: tape.make_engine_loci(e, data, c["scaling"]))
    host = HD.HeredDriver(hostdrv.hip_driver(eng, loci_of(eng), data, seed=31, scaling=c["scaling"]))
    dev = bpp_amd.Sampler(eng, loci_of(eng), data, seed=31, implementation="big" if forced else None)
    ft = (RATE_FT[0], 0.0) if one_call else RATE_FT
    for drv, is_host in ((host, True), (dev, False)):
        rates, h0 = _configure(drv, c, moves, is_host, ft, name == "frogs")
    hd = HD.walk(host, dev, iters, n, 1e-12 if moves == "uniform" else 1e-9, rates=True, one_call=one_call, exact_scalars=moves == "uniform")
    assert dev.kind() == "big"
    assert (hd != h0).any() and (hd > 0).all()
    hp, ha = dev.heredity_counters()
    cnt = dev.locusrate_counters()
    print(f"[big-scalars] {name} {moves}: HRDT {ha}/{hp}, MUI {cnt['mui'][1]}/{cnt['mui'][0]}, MUBAR {cnt['mubar'][1]}/{cnt['mubar'][0]}")
    assert (hp, ha) == host.heredity_counters() and cnt == host.locusrate_counters()
    assert hp == iters*n and 0 < ha < hp
    assert cnt["mui"][0] == iters*n and 0 < cnt["mui"][1] < iters*n
    rd, md = dev.get_locus_rates()
    assert (rd != rates).any()
    if one_call:
        assert cnt["mubar"] == (0, 0) and md == 1.0
    else:
        assert cnt["mubar"][0] == iters
    dev.close(); host.close(); eng.close()


# ------------------------------------------------------------------ 2. scale counters fire under rates
# The rates of the six 24-tip loci of firing.case("big-24"): a rate below 1 shortens every branch (more underflow), one above
# lengthens it; (0.5, 1.5) keeps firing.fires_at_start's conditions on the ORACLE at the start trees' lengths x mu_i — checked on
# the CPU by tests/test_bigsampler_scalars_host.py and again below before anything runs on the device
FIRING_RATES = (0.5, 1.5)


class _rated_firing:
    """firing's oracle takes every length x mu_i for the length of the block (firing.oracle_locus replaced, as
    locusrates.check_state does with the checker's: not re-entrant) -> the data tagged with the rates"""

    def __init__(self, data, mui):
        self.tagged = [dict(d, _mui=float(m)) for d, m in zip(data, mui)]

    def __enter__(self):
        self.plain = firing.oracle_locus
        firing.oracle_locus = lambda d, *a, **k: LR._Rated(self.plain(d, *a, **k), d["_mui"])
        return self.tagged

    def __exit__(self, *exc):
        firing.oracle_locus = self.plain


def check_buffers_scaled(drv, data, loci, mui):
    """checks 8 and 9 of invariants.check_state for loci WITH scale buffers and rates: the root term through the root's scale
    buffer against the oracle's lnL at lengths x mu_i (1e-12), every P-matrix against the oracle's at (t_parent - t_child) mu_i
    (8 ulp or 5e-16), every inner CLV and every scale buffer == the oracle's node update on the device's P-matrices"""
    seen = dict(root_buffer=0.0, pmat_ulps=0.0, pmat_abs=0.0, counters=0)
    for i, d in enumerate(data):
        t = drv.tree(i)
        tips = len(d["seqs"]); nn = 2*tips - 1
        left, right, parent = ([int(x) for x in t[k]][:nn] for k in ("left", "right", "parent"))
        time, root = [float(x) for x in t["time"]][:nn], int(t["root"])
        clv, pmat = [int(x) for x in t["clv"]][:nn], [int(x) for x in t["pmat"]][:nn]
        ol = invariants.oracle_locus(d, None, None, True, None)
        full = ol.full_lnl(left, right, time, root, rate_mui=float(mui[i]))
        loc = loci[i]
        e = rel(loc.root_loglikelihood(clv[root], clv[root] - tips), full)
        seen["root_buffer"] = max(seen["root_buffer"], e)
        assert e < invariants.LNL_TOL, f"locus {i} root buffer {clv[root]}: rel {e:.3e} from the recompute at lengths x {mui[i]!r}"
        dpm = {}
        for v in range(nn):
            if v == root:
                continue
            dpm[v] = loc.get_pmatrix(pmat[v])
            u, a = invariants.ulps(dpm[v], ol.pmat[v]).max(), np.abs(dpm[v] - ol.pmat[v]).max()
            if u <= invariants.PMAT_ULPS:
                seen["pmat_ulps"] = max(seen["pmat_ulps"], u)
            else:
                seen["pmat_abs"] = max(seen["pmat_abs"], a)
            assert u <= invariants.PMAT_ULPS or a < invariants.PMAT_ATOL, \
                f"locus {i} node {v} P-matrix {pmat[v]}: {u:.1f} ulp, {a:.3e} absolute from the oracle's at length {time[parent[v]] - time[v]!r} x {mui[i]!r}"
        oc, osc = {v: ol.clv[v] for v in range(tips)}, {v: None for v in range(tips)}
        for v in O.postorder(left, right, root):
            l, r = left[v], right[v]
            oc[v], osc[v] = O.orc_partial(oc[l], oc[r], dpm[l], dpm[r], osc[l], osc[r], True, ol.order)
            got = loc.get_clv(clv[v])
            assert (got == oc[v]).all(), f"locus {i} node {v} CLV buffer {clv[v]}: differs from the node update of its children's buffers"
            gs = loc.get_scaler(clv[v] - tips)
            assert (gs == osc[v]).all(), f"locus {i} node {v} scale buffer {clv[v] - tips}: differs from the node update's counters"
            seen["counters"] = max(seen["counters"], int(np.max(gs)))
    return seen


@pytest.mark.parametrize("moves,mui_on", [("uniform", False), ("uniform", True), ("program", True)])
def test_scaling_fires_under_rates(moves, mui_on):
    """firing.case("big-24") with rates on FIRING_RATES, fixed or moved by MUI (a narrow gamma(200, 200) on mu_i / mu_bar and a
    window of 0.05, as firing.py narrows its own priors: the chain stays where the counters fire), 30 iterations in chunks
    1 / 3 / 30: before and after every chunk the oracle at lengths x mu_i shows counters that still fire, the state is the CPU's
    recompute (heredity.check_state, rated, scaling) and every device buffer — scale buffers among them — the oracle's"""
    c = firing.case("big-24")
    data, (parent, tau0, thetas0) = c["data"], c["stree"]
    n = len(data)
    mui0 = LR.spread_rates(n, *FIRING_RATES)
    with _rated_firing(data, mui0) as tagged:
        firing.fires_at_start(tagged)
    eng = bpp_amd.Engine(0)
    loci = tape.make_engine_loci(eng, data, True)
    dev = bpp_amd.Sampler(eng, loci, data, seed=31)
    shapes.configure(dev, c, moves)
    dev.set_locus_rates(mui0)
    if mui_on:
        dev.set_locusrate_moves(0.05, 0.0, 200.0)
    dev.initialize()
    assert dev.kind() == "big"
    line, done = [], 0
    for upto in (0, 1, 3, 30):
        dev.iterate(upto - done)
        done = upto
        mui, _ = dev.get_locus_rates()
        HD.check_state(dev, data, parent, rated=True, scaling=True, tip_species=c["species"])
        seen = check_buffers_scaled(dev, data, loci, mui)
        trees = [dev.tree(i) for i in range(n)]
        with _rated_firing(data, mui) as tagged:
            firing.still_fires(tagged, trees)
            line.append(firing.summary(tagged, trees))
        assert seen["counters"] >= 1
    s = dev.summary()
    invariants.moved(dev, tau0, thetas0, s["proposals"], s["accepted"])
    cnt = dev.locusrate_counters()
    print(f"[big-scalars] fires {moves} mui {mui_on}: MUI {cnt['mui']}, rates {list(mui)}; nodes with a counter per locus: "
          + " / ".join(str([x[0] for x in v]) for v in line) + f"; largest counter {[max(x[1] for x in v) for v in line]}; {seen}")
    if mui_on:
        assert cnt["mui"][0] == 30*n and 0 < cnt["mui"][1] < 30*n and (mui != mui0).all()
    else:
        assert cnt["mui"] == (0, 0) and (mui == mui0).all()
    dev.close(); eng.close()


# ------------------------------------------------------------------ 3. the state after a long run
@pytest.mark.parametrize("moves", ["uniform", "program"])
def test_state_invariants_after_a_long_run_with_scalars(moves):
    """200 iterations on big-17-300 with HRDT, MUI and MUBAR on: every locus's stored density is the host driver's one-locus
    density at (tree, taus, thetas, h_i) to 1e-11, its lnl the oracle's at lengths x mu_i to 1e-12, every P-matrix buffer within
    8 ulp or 5e-16 of the oracle's at (t_parent - t_child) mu_i, every inner CLV == the node update of its children's buffers
    (heredity.check_state -> locusrates.check_state / check_buffers); reading twice returns the same"""
    c = dict(shapes.case("big-17-300"), model="jc69")
    data, n = c["data"], len(c["data"])
    eng = bpp_amd.Engine(0)
    loci = tape.make_engine_loci(eng, data)
    dev = bpp_amd.Sampler(eng, loci, data, seed=13)
    rates, h0 = _configure(dev, c, moves, False, RATE_FT, False)
    dev.initialize()
    assert dev.kind() == "big"
    HD.check_state(dev, data, c["stree"][0], rated=True, loci=loci, tip_species=c["species"])
    dev.iterate(200)
    seen = HD.check_state(dev, data, c["stree"][0], rated=True, loci=loci, tip_species=c["species"])
    print(f"[big-scalars] state {moves}: {seen}")
    hc, rc = dev.heredity_counters(), dev.locusrate_counters()
    assert hc[0] == 200*n and 0 < hc[1] < hc[0]
    assert rc["mui"][0] == 200*n and 0 < rc["mui"][1] < 200*n and rc["mubar"][0] == 200 and 0 < rc["mubar"][1] < 200
    h1 = dev.get_heredity()
    r1, m1 = dev.get_locus_rates()
    assert (h1 != h0).all() and (h1 > 0).all() and np.isfinite(h1).all()
    assert (r1 != rates).all() and (r1 > 0).all() and np.isfinite(r1).all() and m1 != 1.0
    s = dev.summary()
    trees = [dev.tree(i) for i in range(n)]
    r2, m2 = dev.get_locus_rates()                                     # read again: nothing ran in between
    assert (dev.get_heredity() == h1).all() and (r2 == r1).all() and m2 == m1
    assert dev.heredity_counters() == hc and dev.locusrate_counters() == rc and dev.summary() == s
    assert [dev.tree(i) for i in range(n)] == trees
    dev.close(); eng.close()


# ------------------------------------------------------------------ 4. prior only
@pytest.mark.parametrize("which", ["heredity", "rates"])
@pytest.mark.parametrize("moves", ["uniform", "program"])
def test_prior_only_run_on_the_big_tree_sampler_leaves_every_prior(moves, which):
    """usedata = 0 on the data, priors, step lengths and run length (500 + 2 000 x 3 iterations) of
    tests/test_gpu_heredity.py::test_prior_only_run_on_the_device_leaves_every_prior, the loci forced onto the big-tree sampler:
    heredity — every h_i ~ gamma(4, 4), every theta and the root's tau their own priors (heredity.prior_marginals); rates —
    mu_bar ~ gamma(10, 10) and every mu_i / mu_bar ~ gamma(5, 5) with the windows of the generic sampler's prior-only test
    (locusrates.prior_marginals).  Same bars: means within 4.5 batch-means standard errors, sd within (0.8, 1.2) of the prior's"""
    stree = synth.species_tree_arrays(4)
    parent, tau0, thetas = stree
    sp = [0, 0, 1, 1, 2, 2, 3, 3]
    data = shapes.shaped_set(sp, stree, [20 + k for k in range(12)], 85, model="gtr", rate_cats=4)
    eng = bpp_amd.Engine(0)
    eng.set_options(usedata=0, bfbeta=1.0)
    dev = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, data), data, seed=17, implementation="big")
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
    if which == "heredity":
        dev.set_heredity_move(1.5, 4.0, 4.0)
    else:
        dev.set_locusrate_moves(1.2, 0.6, 5.0, 10.0, 10.0, 1.0)
    dev.initialize()
    assert dev.kind() == "big"
    try:
        if which == "heredity":
            HD.prior_marginals(dev, dev.iterate, 500, 2000, 3, 4.0, 4.0, (4.0, 1000.0), (ta, tb), [True]*len(parent))
        else:
            LR.prior_marginals(dev, dev.iterate, 500, 2000, 3, 5.0, (10.0, 10.0))
    finally:
        eng.set_options(usedata=1, bfbeta=1.0)
    dev.close(); eng.close()


# ------------------------------------------------------------------ 5. ones change nothing
@pytest.mark.parametrize("moves", ["uniform", "program"])
def test_rates_and_scalars_of_one_change_nothing(moves):
    """x*1.0 == x and h == 1.0 takes the table's log(2/theta): a big-tree sampler with rates and scalars explicitly 1.0 (the
    arrays exist, the kernel loads from them) and the moves off walks the trajectory of one on which nothing was set (null
    pointers, no load) to the bit — summary() with its launch count, taus, thetas, trees, counters"""
    c = dict(shapes.case("big-17-30"), model="jc69")
    n = len(c["data"])
    eng = bpp_amd.Engine(0)
    runs = []
    for touched in (False, True):
        dev = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, c["data"]), c["data"], seed=23)
        LR.configure(dev, c, moves, False, ft=None, rates=np.ones(n) if touched else None)
        if touched:
            dev.set_locusrate_moves(0.0, 0.0, 5.0, 10.0, 10.0, 1.0)
            dev.set_heredity(np.ones(n))
            dev.set_heredity_move(0.0, 4.0, 4.0)
        dev.initialize()
        dev.iterate(10)
        assert dev.kind() == "big"
        runs.append((dev.summary(), dev.taus(), dev.thetas(), [dev.tree(i) for i in range(n)]))
        assert dev.locusrate_counters() == dict(mui=(0, 0), mubar=(0, 0)) and dev.heredity_counters() == (0, 0)
        assert (dev.get_locus_rates()[0] == 1.0).all() and dev.get_locus_rates()[1] == 1.0 and (dev.get_heredity() == 1.0).all()
        dev.close()
    assert runs[0] == runs[1]
    assert runs[0][0]["accepted"] > 0
    eng.close()


# ------------------------------------------------------------------ 6. what stays refused
def test_what_the_big_tree_sampler_refuses():
    c = dict(shapes.case("big-17-30"), model="jc69")
    n = len(c["data"])
    eng = bpp_amd.Engine(0)
    smp = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, c["data"]), c["data"], seed=3)
    LR.configure(smp, c, "uniform", False, ft=None)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(bpp_amd.BpaError, match="> 0 and finite"):
            smp.set_locus_rates([1.0, bad, 1.0])
        with pytest.raises(bpp_amd.BpaError, match="> 0 and finite"):
            smp.set_heredity([1.0, 1.0, bad])
    with pytest.raises(bpp_amd.BpaError, match="a_mui"):
        smp.set_locusrate_moves(0.5, 0.0, 0.0)
    with pytest.raises(bpp_amd.BpaError, match="a_mui"):
        smp.set_locusrate_moves(0.0, 0.5, -1.0, 10.0, 10.0)
    for a, b in ((0.0, 4.0), (4.0, -1.0), (float("nan"), 4.0)):
        with pytest.raises(bpp_amd.BpaError, match="a, b > 0"):
            smp.set_heredity_move(0.5, a, b)
    with pytest.raises(bpp_amd.BpaError, match="width"):
        smp.set_heredity_move(-0.5, 4.0, 4.0)
    smp.set_locus_rates([0.5, 1.0, 2.0])
    smp.set_heredity([0.25, 0.75, 1.0])
    smp.initialize()
    assert smp.kind() == "big"
    with pytest.raises(bpp_amd.BpaError, match="before bpa_sampler_initialize"):
        smp.set_locus_rates(np.ones(n))
    with pytest.raises(bpp_amd.BpaError, match="before bpa_sampler_initialize"):
        smp.set_heredity(np.ones(n))
    assert list(smp.get_locus_rates()[0]) == [0.5, 1.0, 2.0] and list(smp.get_heredity()) == [0.25, 0.75, 1.0]
    smp.set_locusrate_moves(0.5, 0.4, 5.0, 10.0, 10.0, 1.0)
    smp.set_heredity_move(0.5, 4.0, 4.0)
    smp.iterate(1)                                                  # the supported combination runs
    assert smp.heredity_counters()[0] == n and smp.locusrate_counters()["mui"][0] == n and smp.locusrate_counters()["mubar"][0] == 1
    before = smp.summary()["launches"]
    smp.set_allreduce(lambda p, n_, st: 1, 0, 0)
    with pytest.raises(bpp_amd.BpaError, match="one rank"):
        smp.iterate(1)
    assert smp.summary()["launches"] == before                      # refused before anything was launched
    smp.close()
    # a composite still refuses, and names both samplers that accept
    parent, tau0, thetas = synth.species_tree_arrays(8)
    mixed = synth.make_dataset(20, 300, 8, "jc69", 1, seed=5) + synth.make_dataset(6, 300, 8, "gtr", 4, seed=7)
    comp = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, mixed), mixed, seed=3)
    comp.set_species_tree(parent, tau0, thetas)
    for call in (lambda: comp.set_locus_rates(np.full(len(mixed), 1.5)), lambda: comp.set_locusrate_moves(0.5, 0.0, 5.0),
                 lambda: comp.set_heredity(np.full(len(mixed), 0.75)), lambda: comp.set_heredity_move(0.5, 4.0, 4.0)):
        with pytest.raises(bpp_amd.BpaError, match="generic and the big-tree sampler only.*composite.*implementation = BPA_SAMPLER_GENERIC in the options"):
            call()
    assert comp.kind() == "composite"
    comp.close(); eng.close()
