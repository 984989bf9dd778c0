"""Helpers of the per-locus mutation-rate tests (mu_i / mu_bar: prop_locusrate_mui stree.c:9225, prop_locusrate_mubar
stree.c:9770): the host driver's locus-rate calls through ctypes on top of hostdrv.Driver, the state invariants with the
oracle's branch lengths x mu_i, the shapes of the device trajectory tests, the prior-only checks.  Plain module, no fixtures."""
import ctypes as C

import numpy as np

import bpp_amd
from bpp_amd import synth
import hostdrv
import invariants
import oraclelib as O
from common import rel

# the theta marginals' bars of tests/test_gpu_prior.py / tests/test_host_driver.py: mean within Z batch-means standard errors
# (NB batches), sd within SD_BAND of the prior's
NB, Z, SD_BAND = 40, 4.5, (0.8, 1.2)


def _lib():
    L = hostdrv.lib()
    if not getattr(L, "_locusrates", False):
        L.a00_set_locus_rates.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.a00_get_locus_rates.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.a00_get_locus_rates.restype = None
        L.a00_set_locusrate_moves.argtypes = [C.c_void_p] + [C.c_double]*6
        L.a00_locusrate_counters.argtypes = [C.c_void_p, C.POINTER(C.c_ulong), C.POINTER(C.c_ulong)]
        L.a00_locusrate_counters.restype = None
        L._locusrates = True
    return L


class RateDriver:
    """a hostdrv.Driver with the locus-rate calls, under the names bpp_amd.Sampler gives them; everything else is the
    driver's own (attribute access falls through)"""

    def __init__(self, drv):
        self.drv = drv

    def __getattr__(self, name):
        return getattr(self.drv, name)

    def try_set_locus_rates(self, mui):
        a = (C.c_double*self.drv.n)(*[float(x) for x in mui])
        return bool(_lib().a00_set_locus_rates(self.drv.h, a))

    def set_locus_rates(self, mui):
        assert len(mui) == self.drv.n
        assert self.try_set_locus_rates(mui), "a00_set_locus_rates refused"

    def get_locus_rates(self):
        a, m = (C.c_double*self.drv.n)(), C.c_double()
        _lib().a00_get_locus_rates(self.drv.h, a, C.byref(m))
        return np.array(a[:]), m.value

    def try_set_locusrate_moves(self, ft_mui, ft_mubar, a_mui, a_mubar=0.0, b_mubar=0.0, mubar=0.0):
        return bool(_lib().a00_set_locusrate_moves(self.drv.h, ft_mui, ft_mubar, a_mui, a_mubar, b_mubar, mubar))

    def set_locusrate_moves(self, ft_mui, ft_mubar, a_mui, a_mubar=0.0, b_mubar=0.0, mubar=0.0):
        assert self.try_set_locusrate_moves(ft_mui, ft_mubar, a_mui, a_mubar, b_mubar, mubar), "a00_set_locusrate_moves refused"

    def locusrate_counters(self):
        p, a = (C.c_ulong*2)(), (C.c_ulong*2)()
        _lib().a00_locusrate_counters(self.drv.h, p, a)
        return dict(mui=(p[0], a[0]), mubar=(p[1], a[1]))


def reference_driver(data, seed=1):
    return RateDriver(hostdrv.reference_driver(data, seed=seed))


def hip_driver(eng, loci, data, seed=1):
    return RateDriver(hostdrv.hip_driver(eng, loci, data, seed=seed))


def prior_driver(data, seed=1):
    return RateDriver(hostdrv.prior_driver(data, seed=seed))


# ---- the state invariants (tests/invariants.py) with the oracle's branch lengths x mu_i
class _Rated:
    """an oracle locus whose full_lnl takes every length x mu_i; everything else is the wrapped object's own"""

    def __init__(self, ol, mui):
        self._ol, self._mui = ol, mui

    def __getattr__(self, name):
        return getattr(self._ol, name)

    def full_lnl(self, left, right, times, root, rate_mui=None):
        return self._ol.full_lnl(left, right, times, root, rate_mui=self._mui)


def check_state(drv, data, species_parent, loci=None, **kw):
    """invariants.check_state for a sampler whose loci have rates: every likelihood the oracle recomputes is taken at
    (t_parent - t_child) mu_i, mu_i = drv.get_locus_rates() (locus.c:2350); the loci's device buffers are checked here
    (check_buffers), everything else is the checker's own.  (The rate reaches the checker's oracle through the module's
    oracle_locus, replaced for the length of the call: not re-entrant, one check at a time.)"""
    mui, _ = drv.get_locus_rates()
    tagged = [dict(d, _mui=float(m)) for d, m in zip(data, mui)]
    plain = invariants.oracle_locus
    invariants.oracle_locus = lambda d, *a, **k: _Rated(plain(d, *a, **k), d["_mui"])
    try:
        seen = invariants.check_state(drv, tagged, species_parent, **kw)
    finally:
        invariants.oracle_locus = plain
    if loci is not None:
        seen.update(check_buffers(drv, data, loci, mui, subst=kw.get("subst")))
    return seen


def check_buffers(drv, data, loci, mui, subst=None):
    """What the loci's device buffers hold after a download (checks 8 and 9 of invariants.check_state, no scalers), with the
    P-matrices compared twice:
      own     against the oracle's eigen form evaluated from the DEVICE's own eigensystem and category rates at
              (t_parent - t_child) mu_i — same inputs, so what is left is the arithmetic of one expm1 per eigen-term: the
              project's bar, 8 ulp or 5e-16 (invariants.check_state's).  A length that was not scaled, or scaled by a
              stale rate, is off by orders of magnitude here;
      oracle  against the oracle's P-matrix from the locus's parameters — its own eigensystem from the frequencies and
              exchangeabilities, and the DEVICE's category rates where alpha moves (invariants.check_state's rates_of: the
              device's quantiles differ from the host routine's in the last places, 1e-14 - 1e-13 relative, held to their own
              bar by tests/test_gpu_subst_edges.py; at lengths x mu_i x rate of order 1 that alone moves an entry by more
              than 8 ulp — seen: 10 ulp / 5.55e-16 at a scaled length of 1.43 with the host's rates, while `own` held): the
              same bar.  (|W||V|, the conditioning of the eigen form, is reported only: up to 2.0 on these loci.)  The root buffer and the lnl stay against the host routine's rates, at 1e-10.
    -> the largest figures seen, including how far `own` is from the unscaled bar of 8 ulp / 5e-16"""
    lnl_tol = invariants.LNL_TOL_SUBST if subst else invariants.LNL_TOL
    U, A = invariants.PMAT_ULPS, invariants.PMAT_ATOL
    seen = dict(root_buffer=0.0, pmat_ulps=0.0, pmat_abs_scaled=0.0, own_ulps=0.0, own_abs_scaled=0.0, own_abs_beyond_8ulp=0.0, cond=1.0)
    for i, d in enumerate(data):
        t = drv.tree(i)
        tips = len(d["seqs"]); nn = 2*tips - 1
        left, right, parent = ([int(x) for x in t[k]][:nn] for k in ("left", "right", "parent"))
        time, root = [float(x) for x in t["time"]][:nn], int(t["root"])
        clv, pmat = [int(x) for x in t["clv"]][:nn], [int(x) for x in t["pmat"]][:nn]
        ol = invariants.oracle_locus(d, None, None, False, drv.get_subst_model(i) if subst else None)
        full = ol.full_lnl(left, right, time, root, rate_mui=float(mui[i]))
        loc = loci[i]
        e = rel(loc.root_loglikelihood(clv[root], -1), full)
        seen["root_buffer"] = max(seen["root_buffer"], e)
        assert e < lnl_tol, f"locus {i} root buffer {clv[root]}: rel {e:.3e} from the recompute"
        eigen = d.get("model", "jc69") not in ("jc69",) and d.get("states", 4) == 4
        if eigen:
            ev, iev, evals = loc.get_eigen(0)
            scale = np.maximum(1.0, np.abs(iev) @ np.abs(ev))
            drates = loc.get_category_rates()
            seen["cond"] = max(seen["cond"], float(scale.max()))
            if subst:
                seen["rates_rel"] = max(seen.get("rates_rel", 0.0), float(np.abs(drates/ol.rates - 1).max()))
                ol = invariants.oracle_locus(d, None, None, False, drv.get_subst_model(i), drates)
                ol.full_lnl(left, right, time, root, rate_mui=float(mui[i]))
        else:
            scale = 1.0
        dpm = {}
        for v in range(nn):
            if v == root:
                continue
            dpm[v] = loc.get_pmatrix(pmat[v])
            length = (time[parent[v]] - time[v])*float(mui[i])
            if eigen:
                own = O.orc_pmatrix_eigen(drates, length, evals, ev, iev)
                u, a = invariants.ulps(dpm[v], own), np.abs(dpm[v] - own)
                ok = (u <= U) | (a < A)
                assert ok.all(), f"locus {i} node {v} P-matrix {pmat[v]}: {u[~ok].max():.1f} ulp / {a[~ok].max():.3e} from the eigen form of the device's OWN eigensystem at length {length!r} = {time[parent[v]] - time[v]!r} x {mui[i]!r}"
                seen["own_ulps"] = max(seen["own_ulps"], float(u[u <= U].max(initial=0.0)))
                seen["own_abs_scaled"] = max(seen["own_abs_scaled"], float((a/scale)[u > U].max(initial=0.0)))
                seen["own_abs_beyond_8ulp"] = max(seen["own_abs_beyond_8ulp"], float(a[u > U].max(initial=0.0)))
            u, a = invariants.ulps(dpm[v], ol.pmat[v]), np.abs(dpm[v] - ol.pmat[v])
            ok = (u <= U) | (a < A)
            assert ok.all(), f"locus {i} node {v} P-matrix {pmat[v]}: {u[~ok].max():.1f} ulp / {a[~ok].max():.3e} from the oracle's at length {length!r} (|W||V| up to {np.max(scale):.2f})"
            seen["pmat_ulps"] = max(seen["pmat_ulps"], float(u[u <= U].max(initial=0.0)))
            seen["pmat_abs_scaled"] = max(seen["pmat_abs_scaled"], float((a/scale)[u > U].max(initial=0.0)))
        oc = {v: ol.clv[v] for v in range(tips)}
        for v in O.postorder(left, right, root):
            oc[v], _ = O.orc_partial(oc[left[v]], oc[right[v]], dpm[left[v]], dpm[right[v]], None, None, False, ol.order)
            got = loc.get_clv(clv[v])
            assert (got == oc[v]).all(), f"locus {i} node {v} CLV buffer {clv[v]}: differs from the node update of its children's buffers (max abs {np.abs(got - oc[v]).max():.3e})"
    return seen


def oracle_lnl(d, t, mui, params=None):
    """one locus's likelihood from scratch on tree t (a tree() dict) with lengths x mui"""
    ol = invariants.oracle_locus(d, None, None, False, params)
    n = 2*len(d["seqs"]) - 1
    return ol.full_lnl([int(x) for x in t["left"]][:n], [int(x) for x in t["right"]][:n], [float(x) for x in t["time"]][:n], int(t["root"]), rate_mui=float(mui))


def spread_rates(n, lo, hi, seed=3):
    """n rates log-uniform on (lo, hi), not all equal, both ends present"""
    r = np.exp(np.random.default_rng(seed).uniform(np.log(lo), np.log(hi), n))
    r[0], r[-1] = lo, hi
    return r


# ---- shapes
def mixed_host_data():
    """6 JC69 4-tip loci (tips in species A, C, E, G) and 4 GTR+Gamma4 8-tip loci on the 8-species tree ->
    (data, tip species per locus, (parent, tau0, thetas))"""
    parent, tau0, thetas = synth.species_tree_arrays(8)
    small = synth.make_dataset(6, 300, 4, "jc69", 1, seed=61)
    rng = np.random.default_rng(62)
    sp4 = [0, 2, 4, 6]
    for d in small:
        d["left"], d["right"], d["times"], d["root"] = synth.msc_start_tree(sp4, parent, tau0, thetas, rng)
    big = synth.make_dataset(4, 300, 8, "gtr", 4, seed=63)
    return small + big, [sp4]*6 + [list(range(8))]*4, (parent, tau0, thetas)


# ---- prior-only runs: what the marginals of mu_bar and mu_i / mu_bar must be
def gamma_check(x, a, b, what):
    x = np.asarray(x, float)
    m = len(x)//NB
    bm = np.array([x[i*m:(i + 1)*m].mean() for i in range(NB)])
    se = bm.std(ddof=1)/np.sqrt(NB)
    print(f"{what}: mean {x.mean():.5f} (gamma({a}, {b}): {a/b:.5f}, batch se {se:.5f}, z {abs(x.mean() - a/b)/se:.2f}), sd ratio {x.std()/(np.sqrt(a)/b):.3f}")
    assert abs(x.mean() - a/b) < Z*se, (what, x.mean(), a/b, se)
    assert SD_BAND[0] < x.std()/(np.sqrt(a)/b) < SD_BAND[1], (what, x.std(), np.sqrt(a)/b)


def prior_marginals(drv, iterate, burn, samples, thin, a_mui, mubar_prior):
    """run and check: mubar_prior = (a, b): mu_bar ~ gamma(a, b) and every mu_i / mu_bar ~ gamma(a_mui, a_mui); None: mu_bar
    is fixed at 1, the MUBAR counters stay 0 and every mu_i ~ gamma(a_mui, a_mui)"""
    iterate(burn)
    R, M = [], []
    for _ in range(samples):
        iterate(thin)
        r, m = drv.get_locus_rates()
        R.append(r); M.append(m)
    R, M = np.array(R), np.array(M)
    c = drv.locusrate_counters()
    assert 0 < c["mui"][1] < c["mui"][0]
    if mubar_prior is None:
        assert c["mubar"] == (0, 0) and (M == 1.0).all()
    else:
        assert 0 < c["mubar"][1] < c["mubar"][0]
        gamma_check(M, mubar_prior[0], mubar_prior[1], "mu_bar")
    for i in range(R.shape[1]):
        gamma_check(R[:, i]/M, a_mui, a_mui, f"mu_{i}/mu_bar")


# ---- the device trajectory tests' shapes (built once per process, never changed)
_CASES = {}


def case(name, nloci=None):
    """'a': 70 JC69 4-tip loci (more than the 64 loci of a gstep_kernel workgroup); 'b': GTR+Gamma4 8-tip loci of about 30
    patterns (200: two part-batches of the packing); 'c': 12 GTR+Gamma4 16-tip loci, two sequences per species (32-lane groups);
    'd': 130 LG+Gamma4 6-tip loci of 64 patterns (the 20-state records, split into parts)
    -> dict(data, species per locus or None, stree, model)"""
    import shapes
    key = (name, nloci)
    if key in _CASES:
        return _CASES[key]
    if name == "a":
        c = dict(data=synth.make_dataset(nloci or 70, 300, 4, "jc69", 1, seed=81), species=None, stree=synth.species_tree_arrays(4), model="jc69")
    elif name == "b":
        n = nloci or 200
        stree = synth.species_tree_arrays(8)
        c = dict(data=shapes.shaped_set(list(range(8)), stree, [28 + k % 5 for k in range(n)], 82, model="gtr", rate_cats=4), species=None, stree=stree, model="gtr")
    elif name == "c":
        stree = synth.species_tree_arrays(8)
        sp = [k//2 for k in range(16)]
        c = dict(data=shapes.shaped_set(sp, stree, [30 + 3*k for k in range(nloci or 12)], 83, model="gtr", rate_cats=4), species=[sp]*(nloci or 12), stree=stree, model="gtr")
    else:
        data = synth.make_dataset(nloci or 130, 400, 6, "lg", 4, seed=84)
        for d in data:                               # exactly one 64-pattern tile per locus
            assert len(d["weights"]) >= 64
            d["seqs"] = [s[:64] for s in d["seqs"]]; d["weights"] = d["weights"][:64]
        c = dict(data=data, species=None, stree=synth.species_tree_arrays(6), model="lg")
    _CASES[key] = c
    return c


def configure(drv, c, moves, host, subst=False, ft=(0.5, 0.4), a_mui=5.0, mubar_prior=(10.0, 10.0), rates=None):
    """species tree, priors, step lengths, proposal kernel ('uniform' / 'program'), substitution moves, rates and rate moves
    of a trajectory pair: the same calls on the host driver (host=True) and the device sampler"""
    parent, tau0, thetas = c["stree"]
    taxa = (len(parent) + 1)//2
    if moves == "program":
        drv.set_proposal_kernel(1)
        drv.set_program_moves(True, 0.3)
    drv.set_species_tree(parent, tau0, thetas)
    if c["species"] is not None:
        for i, sp in enumerate(c["species"]):
            drv.set_tip_species(i, sp)
    drv.set_tau_prior(3.0, 3.0/tau0[-1])
    if c["model"] == "lg":
        drv.set_theta_prior(2.0, 100.0, 0.004); drv.set_finetune(0.03, 0.05, 0.008, 0.2)
    elif moves == "program":
        drv.set_theta_prior(2.0, 1000.0, 0.0004); drv.set_finetune(0.003, 0.005, 0.0004, 0.05)
    else:
        drv.set_theta_prior(2.0, 1000.0, 0.001); drv.set_finetune(0.003, 0.005, 0.0008, 0.2)
    if subst:
        drv.set_subst_moves(0.3, 0.4, 0.8, 1.0, 1.0)
        for i, d in enumerate(c["data"]):
            if host:
                drv.set_subst_model(i, list(d["freqs"]), list(d["exch"]), 0.5, d["rate_cats"])
            else:
                drv.set_subst_model(i, d["freqs"], d["exch"], 0.5)
    if rates is not None:
        drv.set_locus_rates(rates)
    if ft is not None:
        a, b = mubar_prior if mubar_prior else (0.0, 0.0)
        drv.set_locusrate_moves(ft[0], ft[1], a_mui, a, b, 1.0)
    return taxa


def walk(host, dev, iters, nloci, tol, subst=False, one_call=False):
    """the device sampler against the host driver, iteration by iteration: decisions and counters equal (the two rate moves'
    too), total lnL to 1e-10; at the end trees, populations and buffer indices equal, ages, taus, thetas to `tol`, rates and
    their mean (and the substitution parameters) to 1e-11.
    one_call: the device runs all iterations in ONE iterate call and is read only afterwards.  A getter downloads, and a
    download settles the pending step by a launch of its own: only without one between two iterations is a rate step that
    closes an iteration (mu_bar fixed or its move off) settled INSIDE the next iteration's first proposal launch — the lane
    group's settle of a mode-9 step, the old rate coming back on rejection, the lengths and the fused P-matrix fill after it"""
    host.initialize(); dev.initialize()
    assert rel(dev.summary()["total_lnl"], host.total_lnl()) < 1e-13
    if one_call:
        for it in range(iters):
            host.iterate()
        dev.iterate(iters)
    for it in range(0 if one_call else iters):
        host.iterate(); dev.iterate(1)
        s = dev.summary()
        hp, ha, _ = host.counters()
        assert (s["proposals"], s["accepted"]) == (hp, ha), it
        assert dev.locusrate_counters() == host.locusrate_counters(), (it, dev.locusrate_counters(), host.locusrate_counters())
        assert rel(s["total_lnl"], host.total_lnl()) < 1e-10, it
    s = dev.summary()
    assert (s["proposals"], s["accepted"]) == tuple(host.counters()[:2])
    assert dev.locusrate_counters() == host.locusrate_counters()
    assert rel(s["total_lnl"], host.total_lnl()) < 1e-10
    assert np.allclose(dev.taus(), host.taus(), rtol=tol, atol=0)
    assert np.allclose(dev.thetas(), host.thetas(), rtol=tol, atol=0)
    rd, md = dev.get_locus_rates()
    rh, mh = host.get_locus_rates()
    assert np.allclose(rd, rh, rtol=1e-11, atol=0) and rel(md, mh) < 1e-11, (np.abs(rd/rh - 1).max(), md, mh)
    for i in range(nloci):
        a, b = dev.tree(i), host.tree(i)
        assert a["root"] == b["root"]
        for key in ("left", "right", "parent", "clv", "pmat", "pop"):
            assert [int(x) for x in a[key]] == [int(x) for x in b[key]], (i, key)
        assert np.allclose(a["time"], b["time"], rtol=tol, atol=0)
        assert rel(a["lnl"], b["lnl"]) < 1e-10 and rel(a["logpr"], b["logpr"]) < 10*tol
        if subst:
            fh, qh, ah = host.get_subst_model(i)
            fd, qd, ad = dev.get_subst_model(i)
            assert np.allclose(fd, fh, rtol=1e-11, atol=0) and np.allclose(qd, qh, rtol=1e-11, atol=0) and rel(ad, ah) < 1e-11, i
    return rd, md
