"""Helpers of the heredity-scalar tests (h_i of 'heredity = 1 a b' / 'heredity = 2 file': gtree_update_logprob_contrib
gtree.c:3859, prop_heredity gtree.c:8214): the host driver's heredity calls through ctypes on top of hostdrv.Driver (and of
locusrates.RateDriver: both sets of calls on one object), the state invariants with the MSC density recomputed at
(tree, tau, theta, h_i), the device trajectory walk, the prior-only checks.  Plain module, no fixtures."""
import ctypes as C

import numpy as np

import hostdrv
import invariants
import locusrates as LR
from common import rel


def _lib():
    L = hostdrv.lib()
    if not getattr(L, "_heredity", False):
        L.a00_set_heredity.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.a00_get_heredity.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.a00_get_heredity.restype = None
        L.a00_set_heredity_move.argtypes = [C.c_void_p] + [C.c_double]*3
        L.a00_heredity_counters.argtypes = [C.c_void_p, C.POINTER(C.c_ulong), C.POINTER(C.c_ulong)]
        L.a00_heredity_counters.restype = None
        L._heredity = True
    return L


class HeredDriver(LR.RateDriver):
    """a hostdrv.Driver with the heredity calls (and the locus-rate calls), under the names bpp_amd.Sampler gives them"""

    def try_set_heredity(self, h):
        a = (C.c_double*self.drv.n)(*[float(x) for x in h])
        return bool(_lib().a00_set_heredity(self.drv.h, a))

    def set_heredity(self, h):
        assert len(h) == self.drv.n
        assert self.try_set_heredity(h), "a00_set_heredity refused"

    def get_heredity(self):
        a = (C.c_double*self.drv.n)()
        _lib().a00_get_heredity(self.drv.h, a)
        return np.array(a[:])

    def try_set_heredity_move(self, ft_h, a=0.0, b=0.0):
        return bool(_lib().a00_set_heredity_move(self.drv.h, ft_h, a, b))

    def set_heredity_move(self, ft_h, a=0.0, b=0.0):
        assert self.try_set_heredity_move(ft_h, a, b), "a00_set_heredity_move refused"

    def heredity_counters(self):
        p, a = C.c_ulong(), C.c_ulong()
        _lib().a00_heredity_counters(self.drv.h, C.byref(p), C.byref(a))
        return p.value, a.value


def reference_driver(data, seed=1):
    return HeredDriver(hostdrv.reference_driver(data, seed=seed))


def hip_driver(eng, loci, data, seed=1):
    return HeredDriver(hostdrv.hip_driver(eng, loci, data, seed=seed))


def prior_driver(data, seed=1):
    return HeredDriver(hostdrv.prior_driver(data, seed=seed))


def start_scalars(n, seed=7):
    """n scalars log-uniform on (0.25, 2), both ends present, none exactly 1"""
    return LR.spread_rates(n, 0.25, 2.0, seed=seed)


def msc_logpr(t, tips, species_parent, taus, thetas, tip_species, h):
    """(pop, logpr) of one gene tree from scratch at heredity scalar h: a one-locus host driver with lnL = 0 — the density
    tests/test_heredity_host.py pins to the reference's through scalars of 1 and thetas fl(theta h)"""
    ints = invariants._ints
    data = [dict(seqs=["A"]*tips, left=ints(t["left"])[:2*tips - 1], right=ints(t["right"])[:2*tips - 1],
                 times=[float(x) for x in t["time"]][:2*tips - 1], root=int(t["root"]))]
    drv = prior_driver(data, seed=3)
    try:
        drv.set_species_tree(list(species_parent), list(taus), list(thetas))
        drv.set_tip_species(0, ints(tip_species))
        drv.set_heredity([h])
        if not hostdrv.lib().a00_initialize(drv.h):
            return None, None
        r = drv.tree(0)
        return ints(r["pop"]), r["logpr"]
    finally:
        drv.close()


def check_state(drv, data, species_parent, **kw):
    """invariants.check_state (or, when the loci have rates, locusrates.check_state: pass rated=True) for a sampler whose loci have
    heredity scalars: the MSC density of locus i is recomputed at drv.get_heredity()[i].  The checker asks for one recompute
    per locus, in locus order; the scalar reaches it through the module's msc_recompute, replaced for the length of the call
    (not re-entrant, one check at a time) — the number of recomputes is checked against the number of loci."""
    h = [float(x) for x in drv.get_heredity()]
    rated = kw.pop("rated", False)
    calls = []
    plain = invariants.msc_recompute

    def recompute(t, tips, par, taus, thetas, sp):
        calls.append(1)
        return msc_logpr(t, tips, par, taus, thetas, sp, h[len(calls) - 1])
    invariants.msc_recompute = recompute
    try:
        seen = (LR.check_state if rated else invariants.check_state)(drv, data, species_parent, **kw)
    finally:
        invariants.msc_recompute = plain
    assert len(calls) == len(data)
    return seen


# ---- prior-only runs
def prior_marginals(drv, iterate, burn, samples, thin, a, b, theta_prior, tau_prior, has_theta):
    """run with usedata = 0 and check: every h_i ~ gamma(a, b); every theta that can hold a coalescence ~ its gamma prior; the
    root's tau ~ its gamma prior — locusrates.gamma_check's bars (mean within 4.5 batch-means standard errors, sd within
    (0.8, 1.2) of the prior's)"""
    iterate(burn)
    H, TH, TR = [], [], []
    for _ in range(samples):
        iterate(thin)
        H.append(drv.get_heredity()); TH.append(list(drv.thetas())); TR.append(drv.taus()[-1])
    H, TH, TR = np.array(H), np.array(TH), np.array(TR)
    p, acc = drv.heredity_counters()
    assert p == (burn + samples*thin)*H.shape[1] and 0 < acc < p, (p, acc)
    for i in range(H.shape[1]):
        LR.gamma_check(H[:, i], a, b, f"h_{i}")
    for q in range(TH.shape[1]):
        if has_theta[q]:
            LR.gamma_check(TH[:, q], theta_prior[0], theta_prior[1], f"theta_{q}")
    LR.gamma_check(TR, tau_prior[0], tau_prior[1], "tau_root")


# ---- device sampler against host driver
def configure(drv, c, moves, host, subst=False, rates=False, scalars=None, hrdt=(0.6, 4.0, 4.0)):
    """locusrates.configure (species tree, priors, step lengths, proposal kernel, substitution moves; the rate moves when
    `rates`) + the heredity scalars and the HRDT move: the same calls on the host driver (host=True) and the device sampler"""
    n = len(c["data"])
    taxa = LR.configure(drv, c, moves, host, subst=subst, ft=(0.5, 0.4) if rates else None,
                        rates=LR.spread_rates(n, 0.5, 2.0) if rates else None)
    if scalars is not None:
        drv.set_heredity(scalars)
    if hrdt is not None:
        drv.set_heredity_move(*hrdt)
    return taxa


def walk(host, dev, iters, nloci, tol, subst=False, rates=False, one_call=False, exact_scalars=False):
    """the device sampler against the host driver, iteration by iteration: decisions and both counter pairs equal, total lnL to
    1e-10; at the end trees, populations and buffer indices equal, ages, taus, thetas and the scalars to `tol` (exact_scalars:
    ==, the uniform kernel's h' = |h + ft_h (u - 1/2)| involves no libm), logpr to 1e-11, lnl to 1e-10.
    one_call: the device runs all iterations in ONE iterate call and is read only afterwards"""
    host.initialize(); dev.initialize()
    assert rel(dev.summary()["total_lnl"], host.total_lnl()) < 1e-13
    for i in range(nloci):
        assert rel(dev.tree(i)["logpr"], host.tree(i)["logpr"]) < 1e-11, i

    def level(it):
        s = dev.summary()
        hp, ha, _ = host.counters()
        assert (s["proposals"], s["accepted"]) == (hp, ha), it
        assert dev.heredity_counters() == host.heredity_counters(), (it, dev.heredity_counters(), host.heredity_counters())
        if rates:
            assert dev.locusrate_counters() == host.locusrate_counters(), it
        assert rel(s["total_lnl"], host.total_lnl()) < 1e-10, it
    if one_call:
        for it in range(iters):
            host.iterate()
        dev.iterate(iters)
    else:
        for it in range(iters):
            host.iterate(); dev.iterate(1)
            level(it)
    level(iters)
    p, a = host.heredity_counters()
    assert p == iters*nloci and 0 < a < p, (p, a)
    assert np.allclose(dev.taus(), host.taus(), rtol=tol, atol=0)
    assert np.allclose(dev.thetas(), host.thetas(), rtol=tol, atol=0)
    hd, hh = dev.get_heredity(), host.get_heredity()
    if exact_scalars:
        assert (hd == hh).all(), np.abs(hd/hh - 1).max()
    else:
        assert np.allclose(hd, hh, rtol=tol, atol=0), np.abs(hd/hh - 1).max()
    if rates:
        rd, md = dev.get_locus_rates()
        rh, mh = host.get_locus_rates()
        assert np.allclose(rd, rh, rtol=1e-11, atol=0) and rel(md, mh) < 1e-11
    for i in range(nloci):
        a, b = dev.tree(i), host.tree(i)
        assert a["root"] == b["root"]
        for key in ("left", "right", "parent", "clv", "pmat", "pop"):
            assert [int(x) for x in a[key]] == [int(x) for x in b[key]], (i, key)
        assert np.allclose(a["time"], b["time"], rtol=tol, atol=0)
        assert rel(a["lnl"], b["lnl"]) < 1e-10 and rel(a["logpr"], b["logpr"]) < 1e-11, (i, a["logpr"], b["logpr"])
        if subst:
            fh, qh, ah = host.get_subst_model(i)
            fd, qd, ad = dev.get_subst_model(i)
            assert np.allclose(fd, fh, rtol=1e-11, atol=0) and np.allclose(qd, qh, rtol=1e-11, atol=0) and rel(ad, ah) < 1e-11, i
    return hd
