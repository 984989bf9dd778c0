"""The closed-form DNA models (K80, F81, HKY, T92, TN93, F84) in the device samplers: each model's own parameter steps
(gstep_kernel / gstep2_kernel modes 6 and 7 of csrc/gsampler.hpp, big_step_kernel and big_par_kernel of csrc/bigsampler.hpp;
the table of include/bpp_amd_priors.h), no eigen work for them, the Dirichlet prior on the exchangeabilities
(bpa_sampler_set_qrates_prior) — decision by decision against the C host driver on the same library, the step counts, the
state after a long run against a CPU recompute, GTR with the default prior, and what is refused.
CPU twin: tests/test_closedform_host.py; helpers: tests/closedform.py.  The same models at the edges of their parameters — frequencies
and entries at the moves' floor, kappa from 5e-13 to 2e12, every batched route of the plans, the moves at both ends of their
reflection: tests/test_gpu_closedform_edges.py, tests/test_closedform_edges_host.py, tests/k7.py."""
import numpy as np
import pytest

import bpp_amd
from bpp_amd import synth
import closedform as CF
import firing
import invariants
import locusrates as LR
import shapes
from common import rel

pytestmark = pytest.mark.gpu

S17 = [0, 0, 0] + [k // 2 for k in range(2, 16)]          # 17 tips on 8 species (tests/test_gpu_bigsampler_subst.py's layout)
_SETS = {}


def case(name):
    """the named set, built once and never changed -> the dict locusrates.configure takes (+ models, implementation)"""
    if name in _SETS:
        return _SETS[name]
    st8 = synth.species_tree_arrays(8)
    if name == "gen-hky":
        # 8 loci x 6 tips x 60 patterns, HKY+Gamma4
        st6 = synth.species_tree_arrays(6)
        base = shapes.shaped_set(list(range(6)), st6, [60]*8, 131, model="gtr", rate_cats=4)
        c = dict(data=CF.with_model(base, "hky"), species=None, stree=st6, impl=None)
    elif name == "gen-mixed":
        # K80+Gamma2 / HKY+Gamma4 / TN93+Gamma4 / GTR+Gamma4, two loci each, 8 tips, 28 .. 32 patterns
        base = shapes.shaped_set(list(range(8)), st8, [28 + k % 5 for k in range(8)], 132, model="gtr", rate_cats=4)
        models, cats = ["k80", "k80", "hky", "hky", "tn93", "tn93", "gtr", "gtr"], [2, 2, 4, 4, 4, 4, 4, 4]
        c = dict(data=[CF.recat(d, r) for d, r in zip(CF.with_model(base, models), cats)], species=None, stree=st8, impl=None)
    elif name == "gen-rest":
        # the models the two sets above lack, every locus with several categories (one generic part, no composite):
        # F81+Gamma4 / T92+Gamma4 / F84+Gamma4 / F84+Gamma2, two loci each, 8 tips, 28 .. 32 patterns
        base = shapes.shaped_set(list(range(8)), st8, [28 + k % 5 for k in range(8)], 137, model="gtr", rate_cats=4)
        models, cats = ["f81", "f81", "t92", "t92", "f84", "f84", "f84", "f84"], [4, 4, 4, 4, 4, 4, 2, 2]
        c = dict(data=[CF.recat(d, r) for d, r in zip(CF.with_model(base, models), cats)], species=None, stree=st8, impl=None)
    elif name == "big-17":
        # 6 loci x 17 tips: HKY with ONE category, HKY+Gamma4, TN93+Gamma4, GTR+Gamma4, K80+Gamma2, F84 with one category
        base = shapes.shaped_set(S17, st8, [28 + k % 5 for k in range(6)], 133, model="gtr", rate_cats=4)
        models, cats = ["hky", "hky", "tn93", "gtr", "k80", "f84"], [1, 4, 4, 4, 2, 1]
        c = dict(data=[CF.recat(d, r) for d, r in zip(CF.with_model(base, models), cats)], species=[S17]*6, stree=st8, impl=None)
    elif name in ("big-8-f81", "big-8-t92"):
        # 8-tip loci forced onto the big-tree sampler
        base = shapes.shaped_set(list(range(8)), st8, [28 + k % 5 for k in range(6)], 134, model="gtr", rate_cats=4)
        c = dict(data=CF.with_model(base, name[-3:]), species=None, stree=st8, impl="big")
    else:
        raise KeyError(name)
    c["model"] = "gtr"
    c["models"] = [d["model"] for d in c["data"]]
    c["cats"] = [d["rate_cats"] for d in c["data"]]
    _SETS[name] = c
    return c


def pair(c, seed, moves, prior=CF.PROGRAM_PRIOR, scaling=False, **opts):
    """(engine, host driver, device sampler, the sampler's engine loci) on case c, configured alike"""
    eng = bpp_amd.Engine(0)
    host = CF.hip_driver(eng, c["data"], seed=seed, scaling=scaling)
    loci = CF.make_engine_loci(eng, c["data"], scaling)
    dev = bpp_amd.Sampler(eng, loci, c["data"], seed=seed, implementation=c.get("impl"), **opts)
    for drv, is_host in ((host, True), (dev, False)):
        CF.configure(drv, c, moves, is_host, prior=prior)
    return eng, host, dev, loci


# ------------------------------------------------------------------ 1. decision by decision against the host driver
GENERIC = [
    ("gen-hky", "uniform", {}),
    ("gen-hky", "program", {}),                                # the program's THETA / TAU / MIX decided on the device
    ("gen-hky", "program", dict(host_decisions=True)),
    ("gen-hky", "uniform", dict(chain=True)),                  # GAGE + GSPR as one launch: the parameter step is settled before it
    ("gen-mixed", "uniform", {}),
    ("gen-mixed", "program", {}),
    ("gen-mixed", "program", dict(host_decisions=True)),
    ("gen-rest", "uniform", {}),                               # F81, T92, F84 (kappa = q0/q1): the model == 2, 4, 6 branches of gstep2_kernel
    ("gen-rest", "program", {}),
    ("gen-rest", "program", dict(host_decisions=True)),
    ("gen-rest", "uniform", dict(chain=True)),
]
BIG = [("big-17", "uniform"), ("big-17", "program"), ("big-8-f81", "uniform"), ("big-8-f81", "program"),
       ("big-8-t92", "uniform"), ("big-8-t92", "program")]


def walk_and_check(c, host, dev, moves, kind, iters=4):
    n = len(c["data"])
    tol = 1e-12 if moves == "uniform" else 1e-9
    nfreq, nq = CF.steps_of(c["models"])
    assert dev.subst_steps() == (nfreq, nq)
    LR.walk(host, dev, iters, n, tol, subst=True)
    assert dev.kind() == kind
    moved_f = moved_q = 0
    for i, (d, m) in enumerate(zip(c["data"], c["models"])):
        f, q, alpha = dev.get_subst_model(i)
        assert CF.untouched(m, d["exch"], q), (i, m, q)
        assert max(CF.conserved(m, d["freqs"], d["exch"], f, q)) < 1e-12, (i, m)
        if m == "k80":
            assert list(f) == [0.25]*4
        if d["rate_cats"] == 1:
            assert alpha == 0.5
        moved_f += list(f) != list(d["freqs"]); moved_q += list(q) != list(d["exch"])
    s = dev.summary()
    print(f"[closed-form] {kind} {moves}: frequencies moved on {moved_f} loci, exchangeabilities on {moved_q}; accepted {s['accepted']} of {s['proposals']}, {s['launches']} launches")
    assert (moved_f > 0) == (nfreq > 0) and (moved_q > 0) == (nq > 0)
    assert 0 < s["accepted"] < s["proposals"]


@pytest.mark.parametrize("name,moves,opts", GENERIC, ids=lambda v: shapes.option_id(v) or (v if isinstance(v, str) else "default"))
def test_generic_sampler_equals_host_driver(name, moves, opts):
    """4 iterations, the program's prior {2,4,2,2,4,2}: identical decisions and counters after every iteration, lnL 1e-10, ages,
    taus, thetas 1e-12 (uniform) / 1e-9 (program's moves), parameters 1e-11 (locusrates.walk); the entries a model lacks
    untouched, the sums conserved"""
    c = case(name)
    eng, host, dev, _ = pair(c, 31, moves, **opts)
    walk_and_check(c, host, dev, moves, "generic")
    dev.close(); host.close(); eng.close()


@pytest.mark.parametrize("name,moves", BIG)
def test_big_tree_sampler_equals_host_driver(name, moves):
    """the same on the big-tree sampler: one-category loci next to Gamma loci of four models; forced-big F81 and T92 sets"""
    c = case(name)
    eng, host, dev, _ = pair(c, 37, moves)
    walk_and_check(c, host, dev, moves, "big")
    dev.close(); host.close(); eng.close()


@pytest.mark.parametrize("moves", ["uniform", "program"])
def test_big_tree_sampler_on_firing_data(moves):
    """firing.case("big-24-gtr-g4") declared HKY+Gamma4, with scale buffers: the oracle proves at the HKY start values that the
    counters fire at the start and still fire at the end; 3 iterations next to the host driver (scaling=True), then every
    device buffer — P-matrices against the oracle's closed form at 8 ulp / 5e-16, CLVs and scale counters == — by
    invariants.check_state.  Windows and alpha prior: tests/test_gpu_bigsampler_subst.py's for this set"""
    f0 = firing.case("big-24-gtr-g4")
    data = CF.with_model(f0["data"], "hky")
    c = dict(f0, data=data, subst=False)
    n = len(data)
    tagged = [dict(d, _par=(d["freqs"], d["exch"], 0.5)) for d in data]
    plain = firing.oracle_locus
    firing.oracle_locus = lambda d, model, R, scaling, params, rates=None: plain(d, model, R, scaling, d["_par"], rates)
    try:
        firing.fires_at_start(tagged)
        eng = bpp_amd.Engine(0)
        host = CF.hip_driver(eng, data, seed=31, scaling=True)
        loci = CF.make_engine_loci(eng, data, True)
        dev = bpp_amd.Sampler(eng, loci, data, seed=31)
        for drv, is_host in ((host, True), (dev, False)):
            shapes.configure(drv, c, moves, host=is_host)
            drv.set_subst_moves(0.05, 0.05, 0.05, 200.0, 400.0)
            drv.set_qrates_prior(CF.PROGRAM_PRIOR)
            for i, d in enumerate(data):
                if is_host:
                    drv.set_subst_model(i, list(d["freqs"]), list(d["exch"]), 0.5, d["rate_cats"])
                else:
                    drv.set_subst_model(i, d["freqs"], d["exch"], 0.5)
        assert dev.subst_steps() == (3, 1)
        tol = 1e-12 if moves == "uniform" else 1e-9
        LR.walk(host, dev, 3, n, tol, subst=True)
        assert dev.kind() == "big"
        trees = [dev.tree(i) for i in range(n)]
        now = [dict(d, _par=dev.get_subst_model(i)) for i, d in enumerate(data)]
        firing.still_fires(now, trees)
        print(f"[closed-form] firing {moves}: nodes with a counter / largest counter per locus at the start {firing.summary(tagged)}, at the end {firing.summary(now, trees)}")
    finally:
        firing.oracle_locus = plain
    seen = invariants.check_state(dev, data, c["stree"][0], tip_species=c["species"], scaling=True, loci=loci, subst=True,
                                  rates_of=lambda i: loci[i].get_category_rates())
    print(f"[closed-form] firing {moves}: {seen}")
    dev.close(); host.close(); eng.close()


# ------------------------------------------------------------------ 2. the step counts
def one_iteration(c, on, models=None):
    """a sampler's counters after ONE iteration with the moves on or off (they come last: the tree moves before are the same)"""
    eng = bpp_amd.Engine(0)
    data = c["data"] if models is None else [dict(d, model=m) for d, m in zip(c["data"], models)]
    dev = bpp_amd.Sampler(eng, CF.make_engine_loci(eng, data), data, seed=41, implementation=c.get("impl"))
    CF.configure(dev, c, "uniform", False, prior=CF.PROGRAM_PRIOR, windows=(0.3, 0.4, 0.8) if on else (0.0, 0.0, 0.0))
    steps = dev.subst_steps()
    dev.initialize(); dev.iterate(1)
    s = dev.summary()
    dev.close(); eng.close()
    return steps, s["proposals"], s["launches"]


@pytest.mark.parametrize("name", ["gen-hky", "gen-mixed", "gen-rest", "big-17", "big-8-f81"])
def test_step_counts_equal_the_table(name):
    """subst_steps() and the proposals of an iteration are the table's (HKY: 3 + 1 steps, 5 proposals a locus with Gamma; the
    parent ran 9 steps); the moves off: no steps.  On the all-HKY set declared GTR instead, the iteration has four more steps,
    each at least one launch more"""
    c = case(name)
    want_steps = CF.steps_of(c["models"])
    off_steps, p0, l0 = one_iteration(c, False)
    on_steps, p1, l1 = one_iteration(c, True)
    assert off_steps == (0, 0) and on_steps == want_steps
    assert p1 - p0 == CF.proposals_of(c["models"], c["cats"]), (name, p0, p1)
    if name == "gen-hky":
        assert on_steps == (3, 1) and p1 - p0 == 5*len(c["data"])
        gtr_steps, p2, l2 = one_iteration(c, True, models=["gtr"]*len(c["data"]))
        assert gtr_steps == (3, 5) and p2 - p0 == 9*len(c["data"])
        print(f"[closed-form] launches of the first iteration, 8 loci: moves off {l0}, HKY {l1}, declared GTR {l2}")
        assert l2 - l1 >= 4 and l1 > l0


# ------------------------------------------------------------------ 3. the state after a long run
@pytest.mark.parametrize("name,moves", [("gen-mixed", "uniform"), ("gen-mixed", "program"), ("gen-rest", "program"), ("big-17", "uniform"), ("big-17", "program")])
def test_state_after_300_iterations(name, moves):
    """300 iterations in one call, then invariants.check_state: trees, populations, densities, every lnL against the oracle at
    the current parameters (1e-10), and every device buffer — P-matrices against the oracle's closed form (eigen form for the
    GTR loci) at 8 ulp / 5e-16, CLVs == the node update of their children's buffers"""
    c = case(name)
    eng = bpp_amd.Engine(0)
    loci = CF.make_engine_loci(eng, c["data"])
    dev = bpp_amd.Sampler(eng, loci, c["data"], seed=43, implementation=c.get("impl"))
    CF.configure(dev, c, moves, False, prior=CF.PROGRAM_PRIOR)
    dev.initialize()
    dev.iterate(300)
    seen = invariants.check_state(dev, c["data"], c["stree"][0], tip_species=c["species"], loci=loci, subst=True,
                                  rates_of=lambda i: loci[i].get_category_rates())
    s = dev.summary()
    print(f"[closed-form] {name} {moves} after 300 iterations: {seen}; accepted {s['accepted']} of {s['proposals']}")
    for i, (d, m) in enumerate(zip(c["data"], c["models"])):
        f, q, alpha = dev.get_subst_model(i)
        assert CF.untouched(m, d["exch"], q) and max(CF.conserved(m, d["freqs"], d["exch"], f, q)) < 1e-12, (i, m)
    assert 0 < s["accepted"] < s["proposals"]
    dev.close(); eng.close()


# ------------------------------------------------------------------ 4. GTR with the default prior
@pytest.mark.parametrize("impl", [None, "big"])
def test_gtr_with_the_default_prior_is_the_same_trajectory(impl):
    """GTR+Gamma4 loci: a sampler that sets a prior of ones walks the trajectory (==: counters, trees, parameters, taus, thetas)
    of one that never made the call; with the program's prior the exchangeabilities go elsewhere"""
    c = LR.case("b", 12)
    runs = []
    for prior in (None, CF.FLAT_PRIOR, CF.PROGRAM_PRIOR):
        eng = bpp_amd.Engine(0)
        import tape
        dev = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, c["data"]), c["data"], seed=47, implementation=impl)
        CF.configure(dev, c, "uniform", False, prior=prior)
        assert dev.subst_steps() == (3, 5)
        dev.initialize(); dev.iterate(12)
        n = len(c["data"])
        s = dev.summary()
        runs.append(((s["proposals"], s["accepted"], s["total_lnl"]), list(dev.taus()), list(dev.thetas()),
                     [{k: (list(v) if hasattr(v, "__len__") else v) for k, v in dev.tree(i).items()} for i in range(n)],
                     [tuple(map(lambda x: list(np.atleast_1d(x)), dev.get_subst_model(i))) for i in range(n)]))
        assert dev.kind() == ("big" if impl else "generic")
        dev.close(); eng.close()
    assert runs[0] == runs[1]
    assert runs[2][4] != runs[0][4]


# ------------------------------------------------------------------ 5. refusals
def test_refusals():
    eng = bpp_amd.Engine(0)
    # after initialize
    c = case("gen-hky")
    dev = bpp_amd.Sampler(eng, CF.make_engine_loci(eng, c["data"]), c["data"], seed=3)
    CF.configure(dev, c, "uniform", False, prior=CF.PROGRAM_PRIOR)
    for bad in ([1, 1, 0, 1, 1, 1], [1, 1, 1, 1, 1, float("nan")], [1, -2, 1, 1, 1, 1]):
        with pytest.raises(bpp_amd.BpaError, match="> 0 and finite"):
            dev.set_qrates_prior(bad)
    dev.initialize()
    with pytest.raises(bpp_amd.BpaError, match="before bpa_sampler_initialize"):
        dev.set_qrates_prior(CF.FLAT_PRIOR)
    dev.iterate(1)
    dev.close()
    # a JC69 sampler: the persistent kind and the generic one
    import tape
    jc = synth.make_dataset(8, 300, 4, "jc69", 1, seed=5)
    for impl in (None, "generic"):
        smp = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, jc), jc, seed=3, implementation=impl)
        with pytest.raises(bpp_amd.BpaError, match="the loci are JC69"):
            smp.set_qrates_prior(CF.PROGRAM_PRIOR)
        assert smp.subst_steps() == (0, 0)
        smp.close()
    # one-category non-JC loci: the generic sampler refuses them as before; the big-tree sampler runs them
    one = [CF.recat(d, 1) for d in c["data"]]
    with pytest.raises(bpp_amd.BpaError, match="all have several categories"):
        bpp_amd.Sampler(eng, CF.make_engine_loci(eng, one), one, seed=3)
    big = bpp_amd.Sampler(eng, CF.make_engine_loci(eng, one), one, seed=3, implementation="big")
    CF.configure(big, dict(c, data=one), "uniform", False, prior=CF.PROGRAM_PRIOR)
    assert big.subst_steps() == (3, 1)
    big.initialize(); big.iterate(2)
    assert big.kind() == "big"
    big.close()
    # a big-tree sampler with a JC69 locus among the others still refuses the moves
    st8 = synth.species_tree_arrays(8)
    mixed = CF.with_model(shapes.shaped_set(list(range(8)), st8, [30, 31], 135, model="gtr", rate_cats=4), "hky")
    mixed.append(shapes.shaped_set(list(range(8)), st8, [30], 136)[0])
    smp = bpp_amd.Sampler(eng, CF.make_engine_loci(eng, mixed), mixed, seed=3, implementation="big")
    smp.set_species_tree(*st8)
    smp.set_tau_prior(3.0, 3.0/st8[1][-1]); smp.set_theta_prior(2.0, 1000.0, 0.001); smp.set_finetune(0.003, 0.005, 0.0008, 0.2)
    smp.set_subst_moves(0.3, 0.4, 0.8, 1.0, 1.0)
    for i in range(3):
        smp.set_subst_model(i, [0.25]*4, [1.0]*6, 0.5)
    with pytest.raises(bpp_amd.BpaError, match="need loci with an eigendecomposition"):
        smp.initialize()
    smp.close()
    eng.close()


# ------------------------------------------------------------------ 6. the posterior of the unmodified program
@pytest.mark.parametrize("moves", ["uniform", "program"])
def test_generic_sampler_reproduces_the_programs_hky_posterior(moves):
    """tests/golden/hky_posterior.json (oracle/_ref/bpp, model = hky, alphaprior 1 1 4, two program seeds): the generic sampler
    on the same 12 loci with set_qrates_prior({2,4,2,2,4,2}) — every theta, every tau, lnL and every locus's log kappa: mean
    within 0.3 sd, sd within 0.25 sd of the program's.  moves = "program": BPP's generator, windows and acceptance rule in
    every per-locus move, its THETA / TAU / MIX, the step lengths tuned by its burn-in rule from its defaults"""
    import time
    t0 = time.time()
    data = CF.gold_data()
    c = CF.gold()["config"]
    eng = bpp_amd.Engine(0)
    dev = bpp_amd.Sampler(eng, CF.make_engine_loci(eng, data), data, seed=9)
    if moves == "program":
        dev.set_proposal_kernel(1)
        dev.set_program_moves(True, 0.1)
    CF.gold_setup(dev, data, False, CF.PROGRAM_PRIOR)
    if moves == "program":
        dev.set_theta_prior(c["theta_prior"][0], c["theta_prior"][1], 0.001)       # the program's defaults (bpp.c:530-549)
        dev.set_finetune(5.0, 0.001, 0.001, 0.3)
    dev.initialize()
    assert dev.kind() == "generic" and dev.subst_steps() == (3, 1)
    if moves == "program":
        dev.burnin(2000)
    else:
        dev.iterate(2000)
    rows = []
    for _ in range(5000):
        dev.iterate(2)
        rows.append(CF.gold_row(dev.thetas(), dev.taus(), dev.summary()["total_lnl"], [dev.get_subst_model(i)[1] for i in range(len(data))]))
    misses, worst = CF.gold_compare(rows)
    s = dev.summary()
    print(f"[hky posterior] generic sampler, {moves}: farthest mean {worst[0]:.3f} sd, farthest sd {worst[1]:.3f} sd; accepted {s['accepted']} of {s['proposals']}; {time.time() - t0:.1f} s")
    assert not misses, misses
    dev.close(); eng.close()
