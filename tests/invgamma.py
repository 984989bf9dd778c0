"""Helpers of the inverse-gamma prior tests (BPP's default 'thetaprior = invgamma a b e' / 'tauprior = invgamma a b':
stree.c:3698-3707, 3822, 3865, 5667, 5930-5989; prop_mixing.c:366-423, 502-507): a00_set_prior_kinds and a00_prior_piece bound
on hostdrv.lib(), a driver wrapper with the name bpp_amd.Sampler gives the call, the closed forms in Python, the prior-only
check and the set-up of a trajectory pair.  Plain module, no fixtures."""
import ctypes as C
import math

import numpy as np

import hostdrv
import locusrates as LR

GAMMA, INVGAMMA = 0, 1
KINDS = {"gamma": GAMMA, "invgamma": INVGAMMA}


def lib():
    L = hostdrv.lib()
    if not getattr(L, "_invgamma", False):
        L.a00_set_prior_kinds.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.a00_set_prior_kinds.restype = None
        L.a00_prior_piece.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_double)]
        L.a00_prior_piece.restype = C.c_double
        L.a00_theta_conditional.argtypes = [C.c_double, C.c_double, C.c_long, C.c_double, C.POINTER(C.c_double)]
        L.a00_theta_conditional.restype = None
        L._invgamma = True
    return L


class KindDriver:
    """a hostdrv.Driver (or a wrapper of one) with set_prior_kinds under bpp_amd.Sampler's name and arguments"""

    def __init__(self, drv):
        self.drv = drv

    def __getattr__(self, name):
        return getattr(self.drv, name)

    def set_prior_kinds(self, theta="gamma", tau="gamma"):
        lib().a00_set_prior_kinds(self.drv.h, KINDS.get(theta, theta), KINDS.get(tau, tau))


def piece(which, kind, a, b, *x):
    return lib().a00_prior_piece(which, kind, a, b, (C.c_double*len(x))(*[float(v) for v in x]))


# ---- the closed forms (kind 1), written from the program's statements with math.log / math.lgamma
def theta_prior_lnratio(a, b, to, tn):
    return (-a - 1)*math.log(tn/to) - b*(1/tn - 1/to)


def tau_prior_lnratio(a, b, S, to, tn):
    return (-a - 1 - (S - 1) + 1)*math.log(tn/to) - b*(1/tn - 1/to)


def mix_tau_prior_lnratio(a, b, S, lnc, to, tn):
    return (-a - 1 - (S - 1) + 1)*lnc - b*(1/tn - 1/to)


def theta_lnacc(a, b, k, T, to, tn):
    return k*(math.log(2/tn) - math.log(2/to)) - (T/tn - T/to) + theta_prior_lnratio(a, b, to, tn)


def invgamma_logpdf(x, a, b):
    return a*math.log(b) - math.lgamma(a) - (a + 1)*math.log(x) - b/x


# ---- prior-only runs
def inverse_check(x, a, b, what):
    """x ~ inverse-gamma(a, b)  <=>  1/x ~ gamma(a, b): the inverses are compared, all of whose moments exist (the inverse
    gamma's variance needs a > 2, its fourth moment a > 4) — locusrates.gamma_check's bars"""
    LR.gamma_check(1.0/np.asarray(x, float), a, b, "1/" + what)


def prior_marginals(drv, iterate, burn, samples, thin, theta_prior, tau_prior, has_theta):
    """run with usedata = 0 and check every 1/theta_p that can hold a coalescence and 1/tau_root against gamma(a, b)"""
    iterate(burn)
    TH, TR = [], []
    for _ in range(samples):
        iterate(thin)
        TH.append(list(drv.thetas())); TR.append(drv.taus()[-1])
    TH, TR = np.array(TH), np.array(TR)
    for q in range(TH.shape[1]):
        if has_theta[q]:
            inverse_check(TH[:, q], theta_prior[0], theta_prior[1], f"theta_{q}")
    inverse_check(TR, tau_prior[0], tau_prior[1], "tau_root")


# ---- a trajectory pair (host driver, device sampler): the same calls on both
def configure(drv, stree, species, moves, theta_prior=(3.0, 0.004, 0.001), tau_prior=None, finetune=(0.003, 0.005, 0.0008, 0.2),
              kinds=("invgamma", "invgamma")):
    """inverse-gamma(3, .) priors with their means at the start values (b = (a - 1) x mean); moves: 'uniform' / 'program'"""
    parent, tau0, thetas = stree
    if moves == "program":
        drv.set_proposal_kernel(1)
        drv.set_program_moves(True, 0.3)
    drv.set_species_tree(parent, tau0, thetas)
    if species is not None:
        for i, sp in enumerate(species):
            drv.set_tip_species(i, sp)
    if tau_prior is None:
        tau_prior = (3.0, 2.0*tau0[-1])
    drv.set_tau_prior(*tau_prior)
    drv.set_theta_prior(*theta_prior)
    drv.set_finetune(*finetune)
    if kinds is not None:
        drv.set_prior_kinds(*kinds)


def pair_walk(host, dev, iters, nloci, tol, program):
    """the device sampler against the host driver, iteration by iteration: the decisions' counters equal (with the program's
    moves the Gibbs counters too), total lnL to 1e-10; at the end trees, populations and buffer indices equal, ages, taus and
    thetas to `tol` (1e-12 with uniform windows; 1e-9 with the program's moves, whose T sums are fixed-point on the device and
    whose windows and re-draws go through libm on both sides), every locus's lnL to 1e-10"""
    from common import rel
    host.initialize(); dev.initialize()
    assert rel(dev.summary()["total_lnl"], host.total_lnl()) < 1e-13
    for it in range(iters):
        host.iterate(); dev.iterate(1)
        s = dev.summary()
        hp, ha, _ = host.counters()
        assert (s["proposals"], s["accepted"]) == (hp, ha), it
        assert rel(s["total_lnl"], host.total_lnl()) < 1e-10, it
    gh, gd = tuple(host.gibbs_counters()), tuple(dev.gibbs_counters())
    assert gd == gh, (gd, gh)
    if program:
        assert gd[0] > 0 and gd[1] == gd[0], gd               # every inverse-gamma Gibbs draw is accepted
    assert np.allclose(dev.taus(), host.taus(), rtol=tol, atol=0)
    assert np.allclose(dev.thetas(), host.thetas(), rtol=tol, atol=0)
    for i in range(nloci):
        a, b = dev.tree(i), host.tree(i)
        assert a["root"] == b["root"]
        for key in ("left", "right", "parent", "clv", "pmat", "pop"):
            assert [int(x) for x in a[key]] == [int(x) for x in b[key]], (i, key)
        assert np.allclose(a["time"], b["time"], rtol=tol, atol=0)
        assert rel(a["lnl"], b["lnl"]) < 1e-10 and rel(a["logpr"], b["logpr"]) < 10*tol, (i, a["logpr"], b["logpr"])
