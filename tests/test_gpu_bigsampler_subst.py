"""The substitution-parameter moves on the big-tree device sampler (csrc/bigsampler.hpp: step modes 6 — base frequency k —,
7 — exchangeability k — and 8 — alpha — of big_step_kernel, both instantiations, settled as pend 4; big_par_kernel, which
brings a locus's parameter block and eigensystem level with the sampler's copy; csrc/gsampler_host.hpp: gs_iterate's tail) against
the C host driver on the same library, against the oracle's scale counters at the current parameters, against a CPU
recompute, against the prior, and what is refused.
CPU twin: tests/test_bigsampler_subst_host.py; the generic sampler's tests: tests/test_gpu_gsampler.py, tests/test_gpu_subst_edges.py."""
import numpy as np
import pytest

import bpp_amd
from bpp_amd import synth
import firing
import heredity as HD
import hostdrv
import invariants
import locusrates as LR
import shapes
import tape
from common import rel

pytestmark = pytest.mark.gpu

S17 = [0, 0, 0] + [k // 2 for k in range(2, 16)]          # shapes.case("big-17-...")'s tip layout: 17 tips on 8 species
ALPHA0 = 0.5                                              # locusrates.configure's starting alpha
_SETS = {}


def set17(rate_cats=4):
    """6 GTR loci of 28 .. 32 patterns on the big-17 tip layout, with `rate_cats` categories (built once, never changed)
    -> the dict locusrates.configure takes"""
    if rate_cats not in _SETS:
        stree = synth.species_tree_arrays(8)
        data = shapes.shaped_set(S17, stree, [28 + k % 5 for k in range(6)], 86 + rate_cats, model="gtr", rate_cats=rate_cats)
        _SETS[rate_cats] = dict(data=data, species=[S17]*6, stree=stree, model="gtr", scaling=False)
    return _SETS[rate_cats]


def moved_components(dev, data):
    """per component, the loci on which it differs from its starting value -> (frequencies, exchangeabilities, alpha)"""
    f, q, a = [], [], []
    for i, d in enumerate(data):
        fd, qd, ad = dev.get_subst_model(i)
        if (np.asarray(fd) != np.asarray(d["freqs"], float)).any():
            f.append(i)
        if (np.asarray(qd) != np.asarray(d["exch"], float)).any():
            q.append(i)
        if ad != ALPHA0:
            a.append(i)
    return f, q, a


# ------------------------------------------------------------------ 1. the host driver's trajectory
# set, moves, whole tail (HRDT + MUI + MUBAR on as well), all iterations in one call
TRAJECTORIES = [
    ("17-g4", "uniform", False, False),
    ("17-g4", "program", False, False),
    ("17-g4", "uniform", True, False),                     # HRDT, the nine parameter steps, MUI, MUBAR: a00_iterate's tail
    ("17-g4", "program", True, False),
    ("forced-8-gtr", "program", False, False),             # 8-tip loci forced onto the big-tree sampler (implementation="big")
    ("17-g1", "uniform", False, False),                    # ONE rate category: the alpha move proposes nothing, draws nothing
    ("17-g1", "program", False, False),
    ("17-g4", "uniform", False, True),                     # the alpha step closes the iteration: settled inside the next one's first launch
    ("17-g4", "program", False, True),
]


@pytest.mark.parametrize("name,moves,tail,one_call", TRAJECTORIES)
def test_big_tree_sampler_with_subst_moves_equals_host_driver(name, moves, tail, one_call):
    """3 iterations with the widths and the alpha prior of locusrates.configure (0.3, 0.4, 0.8; gamma(1, 1); alpha starts at
    0.5): decisions and counters equal after every iteration (one_call: at the end), trees, populations and buffer indices
    equal at the end; total lnL 1e-10, ages, taus, thetas 1e-12 with uniform windows and 1e-9 with the program's moves,
    frequencies, exchangeabilities and alpha 1e-11 (locusrates.walk / heredity.walk at their own bars).  Every component moved on
    some locus (one category: alpha on none), and 0 < accepted < proposed"""
    forced = name == "forced-8-gtr"
    c = dict(LR.case("b", 12), scaling=False) if forced else set17(1 if name == "17-g1" else 4)
    data, n = c["data"], len(c["data"])
    eng = bpp_amd.Engine(0)
    host = HD.HeredDriver(hostdrv.hip_driver(eng, tape.make_engine_loci(eng, data), data, seed=31))
    dev = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, data), data, seed=31, implementation="big" if forced else None)
    tol = 1e-12 if moves == "uniform" else 1e-9
    if tail:
        h0 = HD.start_scalars(n)
        for drv, is_host in ((host, True), (dev, False)):
            HD.configure(drv, c, moves, is_host, subst=True, rates=True, scalars=h0)
        HD.walk(host, dev, 3, n, tol, subst=True, rates=True, exact_scalars=moves == "uniform")
        cnt = dev.locusrate_counters()
        assert cnt == host.locusrate_counters() and cnt["mui"][0] == 3*n and cnt["mubar"][0] == 3
    else:
        for drv, is_host in ((host, True), (dev, False)):
            LR.configure(drv, c, moves, is_host, subst=True, ft=None)
        LR.walk(host, dev, 3, n, tol, subst=True, one_call=one_call)
    assert dev.kind() == "big"
    f, q, a = moved_components(dev, data)
    s = dev.summary()
    print(f"[big-subst] {name} {moves} tail {tail} one_call {one_call}: loci whose frequencies / exchangeabilities / alpha moved: "
          f"{f} / {q} / {a}; accepted {s['accepted']} of {s['proposals']}, {s['launches']} launches")
    assert f and q
    if name == "17-g1":
        assert not a                                       # no alpha to move, and the streams stayed level with the host's (the walk)
    else:
        assert a
    assert 0 < s["accepted"] < s["proposals"]
    dev.close(); host.close(); eng.close()


# ------------------------------------------------------------------ 2. scale counters fire under the moves
# firing.case("big-24-gtr-g4"): a moved alpha changes which patterns underflow (a small alpha puts most of a pattern's weight
# on a near-zero rate, whose branches are short: more underflow; a large one the other way).  The widths and the prior keep the
# chain of the REFERENCE-API driver alone where firing.still_fires holds for 20 iterations (tests/test_bigsampler_subst_host.py,
# which runs these very settings on the CPU): windows of 0.05 on the logarithms, as the rated firing test's MUI window, and
# alpha ~ gamma(200, 400) around its starting value of 0.5, as narrow as that test's gamma(200, 200) on mu_i / mu_bar.
FIRING_FT, FIRING_ALPHA_PRIOR = (0.05, 0.05, 0.05), (200.0, 400.0)


class param_firing:
    """firing's oracle takes every locus's CURRENT substitution parameters for the length of the block (firing.oracle_locus
    replaced, as locusrates.check_state does with the checker's: not re-entrant) -> the data tagged with them"""

    def __init__(self, data, params):
        self.tagged = [dict(d, _par=p) for d, p in zip(data, params)]

    def __enter__(self):
        self.plain = firing.oracle_locus
        firing.oracle_locus = lambda d, model, R, scaling, params, rates=None: self.plain(d, model, R, scaling, d["_par"], rates)
        return self.tagged

    def __exit__(self, *exc):
        firing.oracle_locus = self.plain


def configure_firing(drv, c, moves, host):
    """shapes.configure's calls for the firing set (its narrow priors and short steps), then the three moves at FIRING_FT"""
    shapes.configure(drv, c, moves, host=host)
    drv.set_subst_moves(*FIRING_FT, *FIRING_ALPHA_PRIOR)
    for i, d in enumerate(c["data"]):
        if host:
            drv.set_subst_model(i, list(d["freqs"]), list(d["exch"]), ALPHA0, d["rate_cats"])
        else:
            drv.set_subst_model(i, d["freqs"], d["exch"], ALPHA0)


@pytest.mark.parametrize("moves", ["uniform", "program"])
def test_scaling_fires_under_the_subst_moves(moves):
    """firing.case("big-24-gtr-g4"), six 24-tip GTR+Gamma4 loci with scale buffers, all three moves at FIRING_FT with alpha ~
    gamma(200, 400), 3 iterations next to the host driver (scaling=True): before anything runs the oracle proves
    firing.fires_at_start at the starting parameters, after every iteration decisions, counters and the total lnL (1e-10) are
    the host driver's and the oracle at the sampler's CURRENT trees and parameters proves firing.still_fires; at the end the
    trajectory bars of case 1 and every device buffer — P-matrices 8 ulp / 5e-16, CLVs and scale counters == — against the
    oracle (invariants.check_state with scaling, the device's category rates).
    Chosen values: windows (0.05, 0.05, 0.05), alpha ~ gamma(200, 400), alpha starts at 0.5.  The oracle's counters on the
    reference-API driver's chain with them (tests/test_bigsampler_subst_host.py, seed 31, 20 iterations; nodes with a non-zero
    counter per locus / largest counter of the set): start [4, 4, 3, 4, 3, 3] / 2; uniform windows: after 1, 2, 3 iterations
    [3, 4, 5, 4, 4, 3], [3, 4, 4, 3, 3, 3], [3, 4, 3, 3, 2, 3], never below 2 nodes on a locus up to iteration 20 ([4, 5, 6, 5, 3, 3]),
    largest counter 1 throughout; the program's moves: [4, 4, 4, 2, 4, 2], [6, 4, 3, 3, 4, 2], [6, 5, 4, 3, 5, 2], never below 1
    node on a locus up to iteration 20 ([3, 3, 2, 1, 2, 3]), largest counter 1.  Both tests print the figures of their run."""
    c = firing.case("big-24-gtr-g4")
    data, (parent, tau0, thetas0) = c["data"], c["stree"]
    n = len(data)
    start = [(d["freqs"], d["exch"], ALPHA0) for d in data]
    with param_firing(data, start) as tagged:
        firing.fires_at_start(tagged)
        line = [firing.summary(tagged)]
    eng = bpp_amd.Engine(0)
    loci = tape.make_engine_loci(eng, data, True)
    host = LR.RateDriver(hostdrv.hip_driver(eng, tape.make_engine_loci(eng, data, True), data, seed=31, scaling=True))
    dev = bpp_amd.Sampler(eng, loci, data, seed=31)
    configure_firing(host, c, moves, True)
    configure_firing(dev, c, moves, False)
    host.initialize(); dev.initialize()
    assert dev.kind() == "big"
    assert rel(dev.summary()["total_lnl"], host.total_lnl()) < 1e-13
    for it in range(3):
        host.iterate(); dev.iterate(1)
        s = dev.summary()
        assert (s["proposals"], s["accepted"]) == tuple(host.counters()[:2]), it
        assert rel(s["total_lnl"], host.total_lnl()) < 1e-10, it
        trees = [dev.tree(i) for i in range(n)]
        with param_firing(data, [dev.get_subst_model(i) for i in range(n)]) as tagged:
            firing.still_fires(tagged, trees)
            line.append(firing.summary(tagged, trees))
    tol = 1e-12 if moves == "uniform" else 1e-9
    assert np.allclose(dev.taus(), host.taus(), rtol=tol, atol=0) and np.allclose(dev.thetas(), host.thetas(), rtol=tol, atol=0)
    for i in range(n):
        a, b = dev.tree(i), host.tree(i)
        assert a["root"] == b["root"]
        for key in ("left", "right", "parent", "clv", "pmat", "pop"):
            assert [int(x) for x in a[key]] == [int(x) for x in b[key]], (i, key)
        assert np.allclose(a["time"], b["time"], rtol=tol, atol=0)
        assert rel(a["lnl"], b["lnl"]) < 1e-10 and rel(a["logpr"], b["logpr"]) < 10*tol
        fh, qh, ah = host.get_subst_model(i)
        fd, qd, ad = dev.get_subst_model(i)
        assert np.allclose(fd, fh, rtol=1e-11, atol=0) and np.allclose(qd, qh, rtol=1e-11, atol=0) and rel(ad, ah) < 1e-11, i
    seen = invariants.check_state(dev, data, parent, tip_species=c["species"], scaling=True, loci=loci, subst=True,
                                  rates_of=lambda i: loci[i].get_category_rates())
    f, q, a = moved_components(dev, data)
    s = dev.summary()
    print(f"[big-subst] fires {moves}: nodes with a counter per locus / largest counter, start and after each iteration: "
          + "; ".join(f"{[x[0] for x in v]} / {max(x[1] for x in v)}" for v in line) + f"; moved {f} / {q} / {a}; {seen}")
    assert f and q and a and 0 < s["accepted"] < s["proposals"]
    dev.close(); host.close(); eng.close()


# ------------------------------------------------------------------ 3. the state after a longer run
LONG = 300                                                 # iterations: 48 tree steps + 9 parameter steps + the all-loci steps each, about 2 s in all


@pytest.mark.parametrize("moves", ["uniform", "program"])
def test_state_invariants_after_a_long_run_with_subst_moves(moves):
    """LONG iterations on the 17-tip GTR+Gamma4 set with the three parameter moves, HRDT, MUI and MUBAR on: every locus's lnl and
    root term the oracle's at (tree, parameters, lengths x mu_i) to 1e-10 (invariants.LNL_TOL_SUBST), its density the one-locus
    driver's at h_i to 1e-11, every P-matrix within 8 ulp / 5e-16 of the eigen form of the device's own eigensystem and of the
    oracle's from the parameters at the device's category rates, every inner CLV == the node update of its children's
    buffers (heredity.check_state -> locusrates.check_state / check_buffers, subst).  Then a batch evaluation of the loci on
    the settled trees returns the sampler's lnL: the parameter blocks and eigensystems are level after rejected proposals"""
    c = set17(4)
    data, n = c["data"], len(c["data"])
    eng = bpp_amd.Engine(0)
    loci = tape.make_engine_loci(eng, data)
    dev = bpp_amd.Sampler(eng, loci, data, seed=13)
    h0 = HD.start_scalars(n)
    HD.configure(dev, c, moves, False, subst=True, rates=True, scalars=h0)
    dev.initialize()
    assert dev.kind() == "big"
    HD.check_state(dev, data, c["stree"][0], rated=True, loci=loci, tip_species=c["species"], subst=True)
    p0 = dev.summary()["proposals"]
    dev.iterate(LONG)
    seen = HD.check_state(dev, data, c["stree"][0], rated=True, loci=loci, tip_species=c["species"], subst=True)
    s = dev.summary()
    f, q, a = moved_components(dev, data)
    print(f"[big-subst] state {moves}: {seen}; accepted {s['accepted']} of {s['proposals']}; moved {f} / {q} / {a}")
    assert len(f) == n and len(q) == n and len(a) == n
    # the nine parameter steps are counted with the tree moves: more proposals than the gene-tree and all-loci steps can add up to
    assert s["proposals"] - p0 > LONG*(9*n)
    assert 0 < s["accepted"] < s["proposals"]
    for i in range(n):
        fd, qd, ad = dev.get_subst_model(i)
        assert abs(sum(fd) - 1) < 1e-12 and min(fd) >= 1e-5 and min(qd) >= 1e-5 and ad > 0
    # what anybody else computes from the loci's blocks now: the likelihood of the settled trees at the settled parameters
    mui, _ = dev.get_locus_rates()
    for i, d in enumerate(data):
        t = dev.tree(i)
        lnl = batch_lnl(eng, loci[i], d, t, float(mui[i]))
        assert rel(lnl, t["lnl"]) < invariants.LNL_TOL_SUBST, (i, lnl, t["lnl"])
    dev.close(); eng.close()


def batch_lnl(eng, loc, d, t, mui):
    """one locus's likelihood from scratch by the engine (every P-matrix from the locus's parameter block and eigensystem as
    they are on the device, every inner node, the root term), into the tree's OTHER buffers"""
    tips = len(d["seqs"]); nn = 2*tips - 1
    left, right, parent = ([int(x) for x in t[k]][:nn] for k in ("left", "right", "parent"))
    time, root = [float(x) for x in t["time"]][:nn], int(t["root"])
    clv, pmat = [int(x) for x in t["clv"]][:nn], [int(x) for x in t["pmat"]][:nn]
    inner, edges = tips - 1, 2*tips - 2
    oclv = lambda v: clv[v] if v < tips else tips + (clv[v] - tips + inner) % (2*inner)
    opm = lambda v: (pmat[v] + edges) % (2*edges)
    br = [v for v in range(nn) if v != root]
    loc.update_matrices([opm(v) for v in br], [(time[parent[v]] - time[v])*mui for v in br])
    import oraclelib as O
    ops = [(oclv(v), -1, oclv(left[v]), opm(left[v]), -1, oclv(right[v]), opm(right[v]), -1) for v in O.postorder(left, right, root)]
    loc.update_partials(ops)
    return loc.root_loglikelihood(oclv(root), -1)


# ------------------------------------------------------------------ 4. prior only
@pytest.mark.parametrize("moves", ["uniform", "program"])
def test_prior_only_run_leaves_alpha_its_prior_and_the_simplex(moves):
    """usedata = 0 on 6 GTR+Gamma4 8-tip loci forced onto the big-tree sampler, 300 + 2 000 x 2 iterations: every locus's alpha ~
    gamma(4, 8) under a window of 1.5 (locusrates.gamma_check: mean within 4.5 batch-means standard errors, sd within (0.8, 1.2)
    of the prior's); at every sample the frequencies sum to 1 within 1e-12 with every component >= 1e-5, the exchangeabilities
    keep their sum (1e-12 relative) with every moved one >= 1e-5.
    The proposal (param_step; locus.c:2819-2833) reflects the MOVED component into [1e-5, v_j + v_ref]; the reference component
    (T, the A<->G rate) takes up the difference and is bounded by 0 only.  Without data the frequencies' target is flat on the
    simplex, where T < 1e-5 has probability 3e-5: a chain that explores the simplex meets it (seen: T = 3.5e-6 after 500
    iterations at widths of 0.5 under the Bactrian windows) — that is the move, not a fault.  The frequency and exchangeability
    windows here are therefore 0.05: from (0.3, 0.2, 0.2, 0.3) a walk of 4 300 steps of sd 0.05 x 0.29 (uniform) / 0.05 (Bactrian)
    on a logarithm spreads by a factor of e^1 .. e^3.3, four orders of magnitude short of a corner, so the simplex check tests
    the arithmetic (sums kept, reflection bound) and not the chain's luck"""
    stree = synth.species_tree_arrays(4)
    parent, tau0, thetas = stree
    sp = [0, 0, 1, 1, 2, 2, 3, 3]
    data = shapes.shaped_set(sp, stree, [20 + k for k in range(6)], 85, model="gtr", rate_cats=4)
    n = len(data)
    eng = bpp_amd.Engine(0)
    eng.set_options(usedata=0, bfbeta=1.0)
    dev = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, data), data, seed=17, implementation="big")
    if moves == "program":
        dev.set_proposal_kernel(1)
        dev.set_program_moves(True, 0.3)
    dev.set_species_tree(parent, tau0, thetas)
    for i in range(n):
        dev.set_tip_species(i, sp)
        dev.set_subst_model(i, data[i]["freqs"], data[i]["exch"], ALPHA0)
    dev.set_tau_prior(6.0, 6.0/tau0[-1])
    dev.set_theta_prior(4.0, 1000.0, 0.004)
    dev.set_finetune(0.008, 0.008, 0.002, 0.5)
    a, b = 4.0, 8.0
    dev.set_subst_moves(0.05, 0.05, 1.5, a, b)
    dev.initialize()
    assert dev.kind() == "big"
    qsum = float(np.sum(data[0]["exch"]))
    try:
        dev.iterate(300)
        A = []
        for _ in range(2000):
            dev.iterate(2)
            row = []
            for i in range(n):
                fd, qd, ad = dev.get_subst_model(i)
                assert abs(fd.sum() - 1) < 1e-12 and fd.min() >= 1e-5, (i, fd)
                assert abs(qd.sum()/qsum - 1) < 1e-12 and np.delete(qd, 1).min() >= 1e-5 and qd[1] > 0, (i, qd)
                row.append(ad)
            A.append(row)
    finally:
        eng.set_options(usedata=1, bfbeta=1.0)
    A = np.array(A)
    for i in range(n):
        LR.gamma_check(A[:, i], a, b, f"alpha_{i}")
    s = dev.summary()
    assert 0 < s["accepted"] < s["proposals"]
    dev.close(); eng.close()


# ------------------------------------------------------------------ 5. nothing set changes nothing
@pytest.mark.parametrize("moves", ["uniform", "program"])
def test_starting_values_with_all_widths_zero_change_nothing(moves):
    """a big-tree sampler with every locus's starting values set and the three widths 0 walks the trajectory of one that never
    heard of them, to the bit: summary() with its launch count, taus, thetas, trees (lnl, logpr, buffer indices)"""
    c = set17(4)
    n = len(c["data"])
    eng = bpp_amd.Engine(0)
    runs = []
    for touched in (False, True):
        dev = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, c["data"]), c["data"], seed=23)
        LR.configure(dev, c, moves, False, ft=None)
        if touched:
            for i, d in enumerate(c["data"]):
                dev.set_subst_model(i, d["freqs"], d["exch"], ALPHA0)
            dev.set_subst_moves(0.0, 0.0, 0.0, 1.0, 1.0)
        dev.initialize()
        dev.iterate(5)
        assert dev.kind() == "big"
        runs.append((dev.summary(), dev.taus(), dev.thetas(), [dev.tree(i) for i in range(n)]))
        if touched:
            assert moved_components(dev, c["data"]) == ([], [], [])
        dev.close()
    assert runs[0] == runs[1]
    assert runs[0][0]["accepted"] > 0
    eng.close()


# ------------------------------------------------------------------ 6. what is refused
def _held(smp):
    s = smp.summary()
    return s["proposals"], s["accepted"], s["total_lnl"], smp.taus(), smp.thetas()


def test_what_the_big_tree_sampler_refuses_of_the_subst_moves():
    eng = bpp_amd.Engine(0)
    # widths > 0 on JC69 loci: no eigendecomposition to refresh — refused when the run is asked for
    cj = dict(shapes.case("big-17-30"), model="jc69")
    smp = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, cj["data"]), cj["data"], seed=3)
    LR.configure(smp, cj, "uniform", False, ft=None)
    for i in range(len(cj["data"])):
        smp.set_subst_model(i, shapes.GTR_FREQS, shapes.GTR_EXCH, ALPHA0)
    smp.initialize()
    assert smp.kind() == "big"
    smp.set_subst_moves(0.3, 0.4, 0.8, 1.0, 1.0)
    before = _held(smp)
    with pytest.raises(bpp_amd.BpaError, match="eigendecomposition"):
        smp.iterate(1)
    smp.set_subst_moves(0.0, 0.0, 0.0, 1.0, 1.0)
    assert _held(smp) == before                                     # refused before anything was proposed
    smp.iterate(1)                                                  # ... and the sampler runs on without the moves
    smp.close()
    # GTR loci
    c = set17(4)
    data, n = c["data"], len(c["data"])
    smp = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, data), data, seed=3)
    LR.configure(smp, c, "uniform", False, ft=None)
    for bad in (dict(k=n), dict(alpha=0.0), dict(alpha=-1.0), dict(alpha=float("nan"))):
        with pytest.raises(bpp_amd.BpaError, match="bad argument"):
            smp.set_subst_model(bad.get("k", 0), data[0]["freqs"], data[0]["exch"], bad.get("alpha", ALPHA0))
    with pytest.raises(bpp_amd.BpaError, match="no substitution model set"):
        smp.get_subst_model(0)
    # loci without starting values (the generic sampler's refusal, with its message)
    smp.initialize()
    assert smp.kind() == "big"
    smp.set_subst_moves(0.3, 0.4, 0.8, 1.0, 1.0)
    before = _held(smp)
    with pytest.raises(bpp_amd.BpaError, match="bpa_sampler_set_subst_model for every locus"):
        smp.iterate(1)
    assert _held(smp) == before
    smp.close()
    smp = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, data), data, seed=3)
    LR.configure(smp, c, "uniform", False, subst=True, ft=None)
    smp.initialize()
    smp.iterate(1)                                                  # the supported combination runs
    assert smp.kind() == "big"
    # values after initialize
    with pytest.raises(bpp_amd.BpaError, match="before bpa_sampler_initialize"):
        smp.set_subst_model(1, data[1]["freqs"], data[1]["exch"], ALPHA0)
    assert moved_components(smp, data) != ([], [], [])
    # several ranks
    before = _held(smp)
    smp.set_allreduce(lambda p, n_, st: 1, 0, 0)
    with pytest.raises(bpp_amd.BpaError, match="one rank"):
        smp.iterate(1)
    assert _held(smp) == before
    smp.close(); eng.close()
