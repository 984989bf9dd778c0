"""Inverse-gamma theta / tau priors — BPP's defaults, 'thetaprior = invgamma a b e' and 'tauprior = invgamma a b' — in the C host
driver (a00_set_prior_kinds; the arithmetic in include/bpp_amd_host.h):

 1. the pieces against the closed forms of the program's statements, written here with math.log / math.lgamma;
 2. a prior-only run (lnL = 0, BPP's usedata = 0) under both move sets: every 1/theta and 1/tau_root comes out gamma(a, b);
 3. the program's own posterior under these priors (tests/golden/invgamma_posterior.json from
    tests/golden/make_golden_invgamma.py) against the host driver on the REAL reference's locus API.

A driver that took the call and ignored it would read inverse-gamma(3, 0.008) as gamma(3, 0.008): a prior mean of 375, not
0.004 — tests 2 and 3 fail on it by orders of magnitude.  GPU twin: tests/test_gpu_invgamma.py."""
import ctypes as C
import itertools
import json
import math
import os

import numpy as np
import pytest

from bpp_amd import synth
import hostdrv
import oraclelib as O
import invgamma as IG

HERE = os.path.dirname(os.path.abspath(__file__))
POP_OF = {"A,B": 4, "A,B,C": 5, "A,B,C,D": 6}           # synth.species_tree_arrays(4): tips, then children before parents

X = [1e-5, 3e-4, 0.004, 0.07, 1.0]                      # thetas and taus
AB = list(itertools.product([1.5, 3.0, 21.0], [1e-4, 0.004, 2.0]))
KT = list(itertools.product([0, 1, 50], [0.0, 1e-3, 30.0]))
PAIRS = [(x, y) for x in X for y in X if x != y]


def close(got, want, terms):
    """agreement to 1e-12 x the largest term's magnitude: each expression is at most four roundings of terms of that size"""
    big = max(abs(t) for t in terms)
    assert abs(got - want) <= 1e-12*big, (got, want, big)


def test_pieces_against_the_closed_forms():
    n = 0
    for (a, b), (to, tn) in itertools.product(AB, PAIRS):
        L = math.log(tn/to)
        close(IG.piece(0, 1, a, b, to, tn), IG.theta_prior_lnratio(a, b, to, tn), [(a + 1)*L, b/tn, b/to])
        for S in (2, 4, 8):
            close(IG.piece(1, 1, a, b, S, to, tn), IG.tau_prior_lnratio(a, b, S, to, tn), [(a + S)*L, b/tn, b/to])
            # MIX: all taus times c = tn/to; the driver writes the Dirichlet part -(S-2) lnc beside the root's own term
            close(IG.piece(2, 1, a, b, S, L, to, tn), IG.mix_tau_prior_lnratio(a, b, S, L, to, tn), [(a + S)*L, b/tn, b/to])
        for k, T in KT:
            close(IG.piece(3, 1, a, b, k, T, to, tn), IG.theta_lnacc(a, b, k, T, to, tn),
                  [(a + 1)*L, b/tn, b/to, k*math.log(2/tn), k*math.log(2/to), T/tn, T/to])
            n += 1
    assert n == 9*20*9
    # theta's conditional: inverse-gamma(a + k, b + T) exactly — no fit, no special case for T = 0
    for (a, b), (k, T) in itertools.product(AB, KT):
        assert IG.piece(4, 1, a, b, k, T) == a + k and IG.piece(5, 1, a, b, k, T) == b + T
    # the re-draws' proposal density (a00_invgamma_logpdf, unchanged): at the conditional's parameters, in its closed form
    # -- with k = 0, T = 0 it is the prior's own density
    for a, b in AB:
        for x in X:
            close(IG.piece(7, 1, a, b, x), IG.invgamma_logpdf(x, a, b), [a*math.log(b), math.lgamma(a), (a + 1)*math.log(x), b/x])


def test_kind_0_is_the_gamma_form_to_the_bit():
    """kind 0 returns what the existing functions return (==): a00_theta_lnacc, a00_theta_conditional, and the gamma
    expressions of tau_step / mix_step, evaluated here in the driver's order of operations"""
    L = IG.lib()
    for (a, b), (to, tn) in itertools.product(AB, PAIRS):
        lr = math.log(tn/to)
        assert IG.piece(0, 0, a, b, to, tn) == (a - 1)*lr - b*(tn - to)
        for S in (2, 4, 8):
            assert IG.piece(1, 0, a, b, S, to, tn) == (a - 1 - (S - 1) + 1)*lr - b*(tn - to)
            assert IG.piece(2, 0, a, b, S, lr, to, tn) == (a - 1)*lr - b*(tn - to) - float(S - 2)*lr
        for k, T in KT:
            assert IG.piece(3, 0, a, b, k, T, to, tn) == IG.piece(6, 0, a, b, k, T, to, tn)
    for (a, b), (k, T) in itertools.product(AB, KT):
        out = (C.c_double*2)()
        L.a00_theta_conditional(a, b, k, T, out)
        got = (IG.piece(4, 0, a, b, k, T), IG.piece(5, 0, a, b, k, T))
        assert all(g == w or (g != g and w != w) for g, w in zip(got, out)), (a, b, k, T, got, list(out))
    # and the two kinds differ everywhere on the grid
    assert all(IG.piece(0, 0, a, b, to, tn) != IG.piece(0, 1, a, b, to, tn) for (a, b), (to, tn) in itertools.product(AB, PAIRS))


PRIOR_THETA = 0.01          # the prior-only runs' theta scale (see test_prior_only_run_leaves_the_inverse_gamma_priors)
PRIOR_FT_THETA = 0.008      # ... and their theta window


def _several(seed, kernel, nloci=12):
    """4 species x 2 sequences (every theta can hold a coalescence), lnL = 0 -> (driver, species tree arrays)"""
    stree = synth.species_tree_arrays(4, PRIOR_THETA)
    parent, tau0, thetas = stree
    sp = [0, 0, 1, 1, 2, 2, 3, 3]
    rng = np.random.default_rng(60 + seed)
    data = []
    for _ in range(nloci):
        l, r, t, rt = synth.msc_start_tree(sp, parent, tau0, thetas, rng)
        data.append(dict(seqs=["A"]*8, left=l, right=r, times=t, root=rt))
    drv = IG.KindDriver(hostdrv.prior_driver(data, seed=seed))
    return drv, stree, [sp]*nloci


@pytest.mark.parametrize("kernel", [0, 1])
def test_prior_only_run_leaves_the_inverse_gamma_priors(kernel):
    """usedata = 0, 12 loci of 4 species x 2 sequences, GAGE / GSPR / THETA / TAU / MIX on, 1 000 + 4 000 x 3 iterations (the
    run length of tests/test_heredity_host.py's prior check): the gene trees integrate out, so every theta comes out
    inverse-gamma(3, 2 theta_0) and the root's tau inverse-gamma(3, 2 tau_0) (b = (a - 1) x the start value) — checked on the
    inverses against gamma(a, b) (mean within 4.5 batch-means standard errors, sd within (0.8, 1.2) of the prior's).  A wrong
    sign or a missing term in a prior ratio, a conditional other than (a + k, b + T) or a Gibbs draw that is not taken as it
    comes shifts these.  Under the program's moves every Gibbs draw is accepted.

    The scale: theta_0 = 0.01 against tau_0 = 0.003 at the root.  At the other tests' theta_0 = 0.002 the root's tau drags the
    gene nodes of twelve loci with it in every rubber band and 1/tau_root's autocorrelation time came out at 30 to 130 samples
    (host driver, three seeds, five sets of step lengths): 2 000 to 4 000 samples are then 20 to 100 independent ones and the
    sd band +-0.2 is met or missed by chance (ratios 0.70 to 1.20 seen).  With theta_0 = 0.01 most coalescences lie in the root
    population, a rubber band moves few nodes, and eighteen such runs at HALF this length gave 1/tau_root sd ratios 0.87 to
    1.09.  The theta window: the root's theta sees about four coalescences in each of twelve loci, its conditional's sd is
    theta/sqrt(a + k - 2) ~ 0.0014, and a uniform window of 0.008 is ~6 of them (at 0.02 the root's theta stood still for runs
    of samples: sd ratio 1.28 on the device); the other step lengths are tests/test_heredity_host.py's."""
    drv, stree, species = _several(21 + kernel, kernel)
    tau0 = stree[1]
    theta_prior, tau_prior = (3.0, 2.0*PRIOR_THETA), (3.0, 2.0*tau0[-1])
    IG.configure(drv, stree, species, "program" if kernel else "uniform", theta_prior=theta_prior + (PRIOR_FT_THETA,), tau_prior=tau_prior,
                 finetune=(0.008, 0.008, 0.002, 0.5))
    drv.initialize()

    def iterate(n):
        for _ in range(n):
            drv.iterate()
    IG.prior_marginals(drv, iterate, 1000, 4000, 3, theta_prior, tau_prior, [True]*7)
    gp, ga = drv.gibbs_counters()
    if kernel:
        assert gp > 0 and ga == gp, (gp, ga)
    else:
        assert (gp, ga) == (0, 0)
    drv.close()


# ---- the program's posterior
@pytest.fixture(scope="module")
def gold():
    return json.load(open(os.path.join(HERE, "golden", "invgamma_posterior.json")))


def dataset(gold):
    c = gold["config"]
    return synth.make_dataset(c["nloci"], c["sites"], c["taxa"], "jc69", 1, seed=c["seed"], theta=c["theta"])


def setup(drv, gold, program=False):
    """the step lengths of tests/test_heredity_posterior.py (same data)"""
    c = gold["config"]
    stree = synth.species_tree_arrays(c["taxa"], c["theta"])
    IG.configure(drv, stree, None, "program" if program else "uniform",
                 theta_prior=tuple(c["theta_prior"]) + (0.004 if program else 0.008,), tau_prior=tuple(c["tau_prior"]),
                 finetune=(0.004, 0.004, 0.0012, 0.2) if program else (0.006, 0.006, 0.003, 0.8))


def sample(drv, host):
    lnl = drv.total_lnl() if host else drv.summary()["total_lnl"]
    return list(drv.thetas()[4:]) + list(drv.taus()[4:]) + [lnl]


def compare(samples, gold):
    c = gold["config"]
    S = np.array(samples)
    seen = set()
    for name, ref in gold["posterior"].items():
        if name == "lnL":
            x = S[:, 6]
        else:
            kind, _, label = name.split(":")
            x = S[:, POP_OF[label] - 4 + (0 if kind == "theta" else 3)]
        seen.add(name)
        print(f"{name}: mean {x.mean():.6g} (program {ref['mean']:.6g}, {abs(x.mean() - ref['mean'])/ref['sd']:.3f} sd), sd {x.std():.6g} (program {ref['sd']:.6g}, {abs(x.std() - ref['sd'])/ref['sd']:.3f})")
        assert abs(x.mean() - ref["mean"]) < c["tol_mean"]*ref["sd"], (name, x.mean(), ref["mean"], ref["sd"])
        assert abs(x.std() - ref["sd"]) < c["tol_sd"]*ref["sd"], (name, x.std(), ref["sd"])
    assert len(seen) == 7 and (c["tol_mean"], c["tol_sd"]) == (0.3, 0.25)


def test_the_fixture_is_the_program_s_inverse_gamma_run(gold):
    c = gold["config"]
    assert tuple(c["theta_prior"]) == (3.0, 0.008) and tuple(c["tau_prior"]) == (3.0, 0.006)
    assert sum(h.startswith("theta:") for h in gold["columns"]) == 3 and gold["samples"] == c["nsample"]
    assert gold["seed2_worst"]["mean"] < c["tol_mean"] and gold["seed2_worst"]["sd"] < c["tol_sd"]


@pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("program", [False, True])
def test_host_driver_reproduces_bpp_posterior_under_inverse_gamma_priors(gold, program):
    """the C host driver on the reference's locus API, 2 000 + 7 000 iterations thinned by 2 (tests/test_heredity_posterior.py),
    with the uniform windows and with the program's moves, within the bars the program's own second seed meets"""
    data = dataset(gold)
    drv = IG.KindDriver(hostdrv.reference_driver(data, seed=5))
    setup(drv, gold, program)
    drv.initialize()
    S = []
    for it in range(9000):
        drv.iterate()
        if it >= 2000 and it % 2 == 0:
            S.append(sample(drv, True))
    compare(S, gold)
    gp, ga = drv.gibbs_counters()
    assert (gp > 0 and ga == gp) if program else (gp, ga) == (0, 0)
    drv.close()
