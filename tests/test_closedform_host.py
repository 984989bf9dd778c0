"""The closed-form models' parameter moves on the C host driver (a00_set_subst_kind, a00_set_qrates_prior; param_step of
csrc/host/a00_driver.c), on the REAL reference's locus API: the defaults change nothing, every model runs the steps of the
reference's table (locus.c:906-952, 2782, 3197-3229) and nothing else, the Dirichlet prior's term (locus.c:3190, 3301-3304)
is the closed form, and without data the exchangeabilities follow that prior.
GPU twin: tests/test_gpu_closedform.py; helpers: tests/closedform.py."""
import ctypes as C
import math

import numpy as np
import pytest

from bpp_amd import synth
import closedform as CF
import hostdrv
import invariants
import locusrates as LR
import oraclelib as O
from common import rel

needs_ref = pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref not built")
SHAPE = dict(nloci=6, sites=120, taxa=4, R=4)


def case(model, seed=91):
    """6 loci x 4 tips x 120 sites with four rate categories, simulated under `model`"""
    data = synth.make_dataset(SHAPE["nloci"], SHAPE["sites"], SHAPE["taxa"], model, SHAPE["R"], seed=seed)
    return dict(data=data, species=None, stree=synth.species_tree_arrays(SHAPE["taxa"]), model=model)


def state(drv, n):
    return (drv.counters(), drv.taus(), drv.thetas(), [drv.tree(i) for i in range(n)], [drv.get_subst_model(i) for i in range(n)])


@needs_ref
def test_defaults_change_nothing():
    """GTR+Gamma4: a driver told that every locus is GTR and that the prior is all ones walks the trajectory of one that never
    made the calls — decisions, trees, parameters ==; the program's prior walks another"""
    c = case("gtr")
    runs = []
    for calls in (None, "defaults", "program"):
        drv = CF.reference_driver(c["data"], seed=7, kinds=calls is not None)
        CF.configure(drv, c, "uniform", True, prior=None if calls is None else CF.FLAT_PRIOR if calls == "defaults" else CF.PROGRAM_PRIOR)
        drv.initialize()
        for _ in range(25):
            drv.iterate()
        runs.append(state(drv, len(c["data"])))
        drv.close()
    assert runs[0] == runs[1]
    assert runs[2][4] != runs[0][4]


@needs_ref
@pytest.mark.parametrize("model", CF.CLOSED)
def test_step_table_on_the_reference_locus_api(model):
    """proposals per iteration = the table's steps + alpha (HKY 5 a locus, K80 2, F81 4): the first iteration of a driver with
    the moves on against one with them off (they come last: the tree moves before them are the same); after 200 iterations
    the entries the model does not have == their start values, the frequencies' sum and the sum of the model's
    exchangeabilities (every move keeps q_j + q_ref) conserved to 1e-12, and every locus's lnL within 1e-10 of the oracle's
    evaluation from scratch at the current tree and parameters"""
    c = case(model)
    data, n = c["data"], len(c["data"])
    counts = []
    for on in (False, True):
        drv = CF.reference_driver(data, seed=13)
        CF.configure(drv, c, "uniform", True, prior=CF.PROGRAM_PRIOR, windows=(0.3, 0.4, 0.8) if on else (0.0, 0.0, 0.0))
        drv.initialize()
        drv.iterate()
        counts.append(drv.counters()[0])
        if not on:
            drv.close()
    want = CF.proposals_of([model]*n, [SHAPE["R"]]*n)
    nfreq, nq = CF.steps_of([model])
    assert want == n*(nfreq + nq + 1) == n*{"k80": 2, "f81": 4, "hky": 5, "t92": 5, "f84": 5, "tn93": 6}[model]
    assert counts[1] - counts[0] == want, (model, counts, want)
    for _ in range(199):
        drv.iterate()
    p, a, _ = drv.counters()
    assert 0 < a < p
    moved_f = moved_q = 0
    for i, d in enumerate(data):
        f, q, alpha = drv.get_subst_model(i)
        assert CF.untouched(model, d["exch"], q), (i, q)
        df, dq = CF.conserved(model, d["freqs"], d["exch"], f, q)
        assert df < 1e-12 and dq < 1e-12, (i, df, dq)
        assert min(f) > 0 and min(q) > 0 and alpha > 0
        moved_f += list(f) != list(d["freqs"]); moved_q += list(q) != list(d["exch"])
        if model == "k80":
            assert list(f) == [0.25]*4
        t = drv.tree(i)
        full = LR.oracle_lnl(d, t, 1.0, (f, q, alpha))
        assert rel(t["lnl"], full) < 1e-10, (i, t["lnl"], full)
    assert (moved_f > 0) == (nfreq > 0) and (moved_q > 0) == (nq > 0)
    drv.close()


@needs_ref
def test_mixed_models_sit_their_steps_out():
    """K80+G2, HKY+G4, TN93+G4, GTR+G4 and a one-category HKY locus side by side: 3 frequency and 5 exchangeability steps an
    iteration, each locus proposing only its own (1 + 1, 3 + 1 + 1, 3 + 2 + 1, 3 + 5 + 1, 3 + 1 proposals); after 40 iterations
    every locus's foreign entries are untouched, its sums conserved and its lnL the oracle's from scratch"""
    base = synth.make_dataset(5, 120, 4, "gtr", 4, seed=93)
    models, cats = ["k80", "hky", "tn93", "gtr", "hky"], [2, 4, 4, 4, 1]
    data = [CF.recat(d, r) for d, r in zip(CF.with_model(base, models), cats)]
    c = dict(data=data, species=None, stree=synth.species_tree_arrays(4), model="gtr")
    assert CF.steps_of(models) == (3, 5) and CF.proposals_of(models, cats) == 2 + 5 + 6 + 9 + 4
    counts = []
    for on in (False, True):
        drv = CF.reference_driver(data, seed=17)
        CF.configure(drv, c, "uniform", True, prior=CF.PROGRAM_PRIOR, windows=(0.3, 0.4, 0.8) if on else (0.0, 0.0, 0.0))
        drv.initialize(); drv.iterate()
        counts.append(drv.counters()[0])
        drv.close()
    assert counts[1] - counts[0] == 26
    drv = CF.reference_driver(data, seed=17)
    CF.configure(drv, c, "uniform", True, prior=CF.PROGRAM_PRIOR)
    drv.initialize()
    for _ in range(40):
        drv.iterate()
    for i, (d, m) in enumerate(zip(data, models)):
        f, q, alpha = drv.get_subst_model(i)
        assert CF.untouched(m, d["exch"], q) and max(CF.conserved(m, d["freqs"], d["exch"], f, q)) < 1e-12, (i, m)
        t = drv.tree(i)
        assert rel(t["lnl"], LR.oracle_lnl(d, t, 1.0, (f, q, alpha))) < 1e-10, i
        if cats[i] == 1:
            assert alpha == 0.5
    drv.close()


def test_prior_term_is_the_closed_form():
    """a00_qrates_prior_piece (bpp_amd_priors.h's expression as compiled) against the reference's statements in Python, at 1e-12
    x the largest piece; a parameter of exactly 1 contributes nothing, whatever its ratio"""
    H = CF.lib()
    H.a00_qrates_prior_piece.restype = C.c_double
    H.a00_qrates_prior_piece.argtypes = [C.POINTER(C.c_double), C.c_int, C.c_int] + [C.c_double]*4
    rng = np.random.default_rng(5)
    priors = [CF.PROGRAM_PRIOR, (1, 4, 1, 1, 1, 1), (2, 1, 1, 1, 1, 1), (0.5, 7.5, 3, 1.25, 9, 2), CF.FLAT_PRIOR]
    for a in priors:
        arr = (C.c_double*6)(*a)
        for ref, js in ((1, (0, 2, 3, 4, 5)), (2, (0, 1))):
            for j in js:
                for _ in range(20):
                    s = math.exp(rng.uniform(-3, 3))
                    x0, x1 = rng.uniform(1e-4, 1 - 1e-4, 2)
                    qo, qn = s*x0, s*x1
                    got = H.a00_qrates_prior_piece(arr, j, ref, qo, qn, s - qo, s - qn)
                    p1, p2 = (a[j] - 1)*(math.log(qn) - math.log(qo)), (a[ref] - 1)*math.log((s - qn)/(s - qo))
                    want = CF.qrates_prior_lnratio(a, j, ref, qo, qn, s - qo, s - qn)
                    assert abs(got - want) <= 1e-12*max(abs(p1), abs(p2), 1e-300), (a, j, ref, got, want)
    assert H.a00_qrates_prior_piece((C.c_double*6)(*CF.FLAT_PRIOR), 0, 1, 0.3, 0.6, 0.7, 0.0) == 0.0      # (not 0 x log 0)


def beta_check(x, a, b, what):
    """LR.gamma_check's bars for a Beta(a, b) sample: mean within Z batch-means standard errors, sd within SD_BAND"""
    x = np.asarray(x, float)
    m = len(x)//LR.NB
    bm = np.array([x[i*m:(i + 1)*m].mean() for i in range(LR.NB)])
    se = bm.std(ddof=1)/np.sqrt(LR.NB)
    mean, sd = a/(a + b), math.sqrt(a*b/((a + b)**2*(a + b + 1)))
    print(f"{what}: mean {x.mean():.5f} (Beta({a}, {b}): {mean:.5f}, batch se {se:.5f}, z {abs(x.mean() - mean)/se:.2f}), sd ratio {x.std()/sd:.3f}")
    assert abs(x.mean() - mean) < LR.Z*se, (what, x.mean(), mean, se)
    assert LR.SD_BAND[0] < x.std()/sd < LR.SD_BAND[1], (what, x.std(), sd)


PARAM_NOOP = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint, C.c_int, C.POINTER(C.c_double), C.c_uint)(lambda *a: 1)


@pytest.mark.parametrize("model,prior", [("hky", CF.PROGRAM_PRIOR), ("tn93", CF.PROGRAM_PRIOR), ("gtr", CF.PROGRAM_PRIOR), ("hky", CF.FLAT_PRIOR)])
def test_without_data_the_exchangeabilities_follow_the_dirichlet(model, prior):
    """usedata = 0 (lnL = 0 for every proposal): the model's entries over their sum are Dirichlet(a), so entry j's share is
    Beta(a_j, sum of the others').  HKY: q_0/(q_0 + q_1) ~ Beta(2, 4); TN93: shares of entries 0, 1, 2 ~ Beta(2, 6), Beta(4, 4),
    Beta(2, 6); GTR: entry j ~ Beta(a_j, 16 - a_j); with the flat prior HKY's share is Beta(1, 1).  The project's bars: mean
    within 4.5 batch-means standard errors, sd within (0.8, 1.2)"""
    n = 4
    base = synth.make_dataset(n, 60, 4, "gtr", 1, seed=95)
    data = CF.with_model(base, model)
    drv = CF.KindDriver(hostdrv.prior_driver(data, seed=23))
    drv.set_param_backend(C.cast(PARAM_NOOP, C.c_void_p))
    parent, tau0, thetas = synth.species_tree_arrays(4)
    drv.set_species_tree(parent, tau0, thetas)
    drv.set_tau_prior(3.0, 3.0/tau0[-1]); drv.set_theta_prior(2.0, 1000.0, 0.001); drv.set_finetune(0.003, 0.005, 0.0008, 0.2)
    nq = CF.TABLE[model][0]
    start = np.ones(6)
    for i in range(n):
        drv.set_subst_model(i, [0.25]*4, list(start), 0.5, 1)
        drv.set_subst_kind(i, model)
    drv.set_subst_moves(0.0, 4.0, 0.0)
    drv.set_qrates_prior(prior)
    drv.initialize()
    for _ in range(500):
        drv.iterate()
    X = []
    for _ in range(16000):
        drv.iterate()
        X.append([drv.get_subst_model(i)[1] for i in range(n)])
    X = np.array(X)                                            # [sample][locus][6]
    assert (X[:, :, nq:] == 1.0).all() and np.allclose(X[:, :, :nq].sum(2), float(nq), rtol=1e-12, atol=0)
    atot = sum(prior[:nq])
    for i in range(n):
        for j in range(nq):
            beta_check(X[:, i, j]/nq, prior[j], atot - prior[j], f"{model} locus {i} q_{j}/sum")
    drv.close()


# ---- the posterior of the unmodified program (tests/golden/hky_posterior.json: make_golden_hky.py, two program seeds)
def host_posterior(prior, iters=14000, burn=2000):
    data = CF.gold_data()
    drv = CF.reference_driver(data, seed=5)
    CF.gold_setup(drv, data, True, prior)
    drv.initialize()
    rows = []
    for it in range(iters):
        drv.iterate()
        if it >= burn and it % 2 == 0:
            rows.append(CF.gold_row(drv.thetas(), drv.taus(), drv.total_lnl(), [drv.get_subst_model(i)[1] for i in range(len(data))]))
    p, a, _ = drv.counters()
    drv.close()
    return rows, a/p


@needs_ref
def test_host_driver_reproduces_the_programs_hky_posterior():
    """12 loci x 4 species x 300 sites, HKY+Gamma4, alphaprior 1 1 4: the host driver on the reference's locus API with
    set_qrates_prior({2,4,2,2,4,2}) against oracle/_ref/bpp — every theta, every tau, lnL and every locus's log kappa: mean
    within 0.3 sd, sd within 0.25 sd of the program's"""
    rows, rate = host_posterior(CF.PROGRAM_PRIOR)
    misses, worst = CF.gold_compare(rows)
    print(f"[hky posterior] host driver, program's prior: farthest mean {worst[0]:.3f} sd, farthest sd {worst[1]:.3f} sd; acceptance {rate:.3f}")
    assert not misses, misses
    assert 0.15 < rate < 0.9
