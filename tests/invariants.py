"""State invariants of a sampler at ANY iteration count (plain helper module, no fixtures).

Everything a sampler holds per locus — tree, buffer indices, population labels, the MSC log-density `logpr`, the
log-likelihood `lnl` — is a function of (tree, taus, thetas, substitution parameters).  check_state recomputes all of it
from scratch on the CPU (oraclelib.OracleLocus, a one-locus hostdrv.prior_driver) and compares; with the engine loci it
also reads every device buffer the tree names and compares it with the oracle's.  Unlike the trajectory tests it needs no
second run next to the one under test, so it holds after any number of iterations.

Works on anything with tree(i) / taus() / thetas(): bpp_amd.Sampler and hostdrv.Driver.

Bars (the project's own; none is fitted to what a device shows):
  lnl, root buffer   1e-12 relative (tests/test_gpu_sampler.py, tests/test_gpu_gsampler.py), 1e-10 with parameter moves
  logpr, total       1e-11 relative (tests/test_gpu_sampler.py; walk() of tests/test_gpu_gsampler.py)
  P-matrices         8 ulp or 5e-16 absolute (tests/test_gpu_parity.py)
  inner CLVs, scale counters: == the oracle's node update on the DEVICE's P-matrices
"""
import numpy as np

import bpp_amd
import hostdrv
import oraclelib as O
from common import rel

LNL_TOL, LNL_TOL_SUBST = 1e-12, 1e-10
LOGPR_TOL = TOTAL_TOL = 1e-11
PMAT_ULPS, PMAT_ATOL = 8, 5e-16


def ulps(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.maximum(np.spacing(np.maximum(np.abs(a), np.abs(b))), 1e-320)


def _ints(a):
    return [int(x) for x in a]


def msc_recompute(t, tips, species_parent, taus, thetas, tip_species):
    """(pop, logpr) of one gene tree from scratch: a one-locus driver with lnL = 0, whose start-up density is pinned
    bit-exact to the reference's gtree_logprob (tests/test_msc_density.py: one_locus_driver)"""
    data = [dict(seqs=["A"] * tips, left=_ints(t["left"]), right=_ints(t["right"]), times=[float(x) for x in t["time"]],
                 root=int(t["root"]))]
    drv = hostdrv.prior_driver(data, seed=3)
    try:
        drv.set_species_tree(list(species_parent), list(taus), list(thetas))
        drv.set_tip_species(0, _ints(tip_species))
        if not hostdrv.lib().a00_initialize(drv.h):
            return None, None
        r = drv.tree(0)
        return _ints(r["pop"]), r["logpr"]
    finally:
        drv.close()


def oracle_locus(d, model, R, scaling, params, rates=None):
    model = d.get("model", "jc69") if model is None else model
    R = d.get("rate_cats", 1) if R is None else R
    S = d.get("states", 4)
    if params is not None:
        f, q, a = params
        return O.OracleLocus(S, R, d["seqs"], d["weights"], model=model, freqs=np.asarray(f, float), qrates=np.asarray(q, float),
                             rates=bpp_amd.compute_gamma_cats(a, a, R) if rates is None else rates, scaling=scaling)
    return O.OracleLocus(S, R, d["seqs"], d["weights"], model=model, freqs=None if model == "jc69" else d["freqs"],
                         qrates=None if model == "jc69" else d["exch"], rates=d.get("rates"), scaling=scaling)


def oracle_root_term(ol, d, clv, scaler):
    """locus_root_loglikelihood on a root CLV: with the phase averaging of an unphased diploid locus when the data has it"""
    dip = d.get("diploid")
    if dip is None:
        return O.orc_lnl(clv, ol.freqs, ol.rw, ol.weights, scaler, ol.order)
    assert scaler is None
    return O.orc_diploid_lnl(O.orc_lhvec(clv, ol.freqs, ol.rw, ol.order), dip["resolution_count"], dip["mapping"], dip["unphased_weights"])


def total_lnl(drv):
    return drv.summary()["total_lnl"] if hasattr(drv, "summary") else drv.total_lnl()


def check_state(drv, data, species_parent, tip_species=None, model=None, R=None, scaling=False, loci=None, subst=None, worst=None,
                rates_of=None):
    """Assert every invariant on every locus; returns the largest differences seen (also merged into `worst` when given):
    dict(lnl, logpr, total, root_buffer, pmat_ulps, pmat_abs).  model / R: None = each locus's own (data[i]["model"],
    ["rate_cats"]); subst: the loci's substitution parameters move — the oracle takes drv.get_subst_model(i); loci: the
    engine loci the sampler was built on — their buffers are read too (after the getters, which download); rates_of (with
    subst): locus number -> the category rates the oracle takes instead of the host routine's for the locus's alpha, or None
    for the host routine's — the DEVICE's own (Locus.get_category_rates) for the loci whose alpha is so large that their last
    places, held to their own bar by the caller, reach a P-matrix entry beyond the P-matrix bar."""
    n = len(data)
    taus, thetas = [float(x) for x in drv.taus()], [float(x) for x in drv.thetas()]
    par = _ints(species_parent)
    npop = len(par)
    S = (npop + 1) // 2
    seen = dict(lnl=0.0, logpr=0.0, total=0.0, root_buffer=0.0, pmat_ulps=0.0, pmat_abs=0.0)
    # 3. species tree
    assert len(taus) == npop and len(thetas) == npop, "species tree: taus / thetas of another size"
    for p in range(npop):
        assert np.isfinite(taus[p]) and np.isfinite(thetas[p]) and thetas[p] > 0, f"population {p}: theta {thetas[p]} / tau {taus[p]}"
        if p < S:
            assert taus[p] == 0.0, f"population {p}: tip tau {taus[p]}"
        if par[p] >= 0:
            assert taus[p] < taus[par[p]], f"population {p}: tau {taus[p]} not below its parent's {taus[par[p]]}"
    anc = []                                              # anc[p]: p and its ancestors
    for p in range(npop):
        a, q = set(), p
        while q >= 0:
            a.add(q); q = par[q]
        anc.append(a)
    lnl_tol = LNL_TOL_SUBST if subst else LNL_TOL
    held_sum = 0.0
    trees = [drv.tree(i) for i in range(n)]
    total = total_lnl(drv)
    for i, d in enumerate(data):
        t = trees[i]
        tips = len(d["seqs"])
        nn, inner, edges = 2 * tips - 1, tips - 1, 2 * tips - 2
        left, right, parent = _ints(t["left"])[:nn], _ints(t["right"])[:nn], _ints(t["parent"])[:nn]
        time, root = [float(x) for x in t["time"]][:nn], int(t["root"])
        clv, pmat, pop = _ints(t["clv"])[:nn], _ints(t["pmat"])[:nn], _ints(t["pop"])[:nn]
        sp = list(range(tips)) if tip_species is None else _ints(tip_species[i])
        # 1. tree shape
        assert tips <= root < nn and parent[root] == -1, f"locus {i}: root {root} has parent {parent[root]}"
        kids = {}
        for v in range(nn):
            if v < tips:
                assert left[v] < 0 and right[v] < 0, f"locus {i} node {v}: a tip with children"
                assert time[v] == 0.0, f"locus {i} node {v}: tip age {time[v]}"
                assert clv[v] == v, f"locus {i} node {v}: tip CLV index {clv[v]}"
            else:
                l, r = left[v], right[v]
                assert 0 <= l < nn and 0 <= r < nn and l != r, f"locus {i} node {v}: children {l}, {r}"
                for c in (l, r):
                    assert c not in kids, f"locus {i} node {c}: child of both {kids.get(c)} and {v}"
                    kids[c] = v
                    assert parent[c] == v, f"locus {i} node {c}: parent {parent[c]}, but it is a child of {v}"
                    assert time[c] < time[v], f"locus {i} node {c}: age {time[c]} not below its parent {v}'s {time[v]}"
            if v != root:
                p = parent[v]
                assert tips <= p < nn and v in (left[p], right[p]), f"locus {i} node {v}: parent {p} does not have it as a child"
        assert len(kids) == nn - 1 and root not in kids, f"locus {i}: not a tree ({len(kids)} child links)"
        reach = O.postorder(left, right, root)
        assert sorted(reach) == list(range(tips, nn)), f"locus {i}: inner nodes reached from the root: {sorted(reach)}"
        # 2. buffer indices
        ci = [clv[v] for v in range(tips, nn)]
        assert all(tips <= c < tips + 2 * inner for c in ci), f"locus {i}: inner CLV index out of range: {ci}"
        assert len(set(ci)) == len(ci), f"locus {i}: two inner nodes share a CLV index: {ci}"
        pi = [pmat[v] for v in range(nn) if v != root]
        assert all(0 <= m < 2 * edges for m in pi), f"locus {i}: P-matrix index out of range: {pi}"
        assert len(set(pi)) == len(pi), f"locus {i}: two nodes share a P-matrix index: {pi}"
        # 4. populations
        for v in range(nn):
            pv = pop[v]
            assert 0 <= pv < npop, f"locus {i} node {v}: population {pv}"
            if v < tips:
                assert pv == sp[v], f"locus {i} node {v}: tip population {pv}, species {sp[v]}"
                continue
            assert taus[pv] <= time[v], f"locus {i} node {v}: age {time[v]} below its population {pv}'s tau {taus[pv]}"
            assert par[pv] < 0 or time[v] < taus[par[pv]], f"locus {i} node {v}: age {time[v]} beyond the end of population {pv} ({taus[par[pv]]})"
            for c in (left[v], right[v]):
                assert pv in anc[pop[c]], f"locus {i} node {v}: population {pv} is no ancestor of child {c}'s {pop[c]}"
        # 5. MSC density
        want_pop, want_logpr = msc_recompute(t, tips, par, taus, thetas, sp)
        assert want_pop is not None, f"locus {i}: the tree does not fit the species tree (the MSC density refuses it)"
        assert pop == want_pop, f"locus {i} pop: held {pop}, recomputed {want_pop}"
        e = rel(t["logpr"], want_logpr)
        seen["logpr"] = max(seen["logpr"], e)
        assert e < LOGPR_TOL, f"locus {i} logpr: held {t['logpr']!r}, recomputed {want_logpr!r} (rel {e:.3e})"
        # 6. likelihood
        ol = oracle_locus(d, model, R, scaling, drv.get_subst_model(i) if subst else None, rates_of(i) if subst and rates_of else None)
        full = ol.full_lnl(left, right, time, root)
        if d.get("diploid") is not None:
            full = oracle_root_term(ol, d, ol.clv[root], ol.scaler[root])
        e = rel(t["lnl"], full)
        seen["lnl"] = max(seen["lnl"], e)
        assert e < lnl_tol, f"locus {i} lnl: held {t['lnl']!r}, recomputed {full!r} (rel {e:.3e})"
        held_sum += t["lnl"]
        if loci is None:
            continue
        # 8. root buffer
        loc = loci[i]
        have = loc.root_loglikelihood(clv[root], clv[root] - tips if scaling else -1)
        e = rel(have, full)
        seen["root_buffer"] = max(seen["root_buffer"], e)
        assert e < lnl_tol, f"locus {i} root buffer {clv[root]}: holds {have!r}, recomputed {full!r} (rel {e:.3e})"
        # 9. inner buffers: the P-matrices against the oracle's, then the CLVs against the oracle's node update on the
        # DEVICE's P-matrices — a stale P-matrix fails the first, a stale CLV the second
        dpm = {}
        for v in range(nn):
            if v == root:
                continue
            dpm[v] = loc.get_pmatrix(pmat[v])
            u, a = ulps(dpm[v], ol.pmat[v]).max(), np.abs(dpm[v] - ol.pmat[v]).max()
            if u <= PMAT_ULPS:
                seen["pmat_ulps"] = max(seen["pmat_ulps"], u)
            else:                                    # (more ulps on entries near zero: the absolute bar decides)
                seen["pmat_abs"] = max(seen["pmat_abs"], a)
            assert u <= PMAT_ULPS or a < PMAT_ATOL, f"locus {i} node {v} P-matrix {pmat[v]}: {u:.1f} ulp, {a:.3e} absolute from the oracle's for branch length {time[parent[v]] - time[v]!r}"
        oc, osc = {v: ol.clv[v] for v in range(tips)}, {v: None for v in range(tips)}
        for v in reach:
            l, r = left[v], right[v]
            oc[v], osc[v] = O.orc_partial(oc[l], oc[r], dpm[l], dpm[r], osc[l], osc[r], scaling, ol.order)
            got = loc.get_clv(clv[v])
            assert (got == oc[v]).all(), f"locus {i} node {v} CLV buffer {clv[v]}: differs from the node update of its children's buffers (max abs {np.abs(got - oc[v]).max():.3e})"
            if scaling:
                gs = loc.get_scaler(clv[v] - tips)
                assert (gs == osc[v]).all(), f"locus {i} node {v} scale buffer {clv[v] - tips}: differs from the node update's counters"
    # 7. total
    e = rel(total, held_sum)
    seen["total"] = e
    assert e < TOTAL_TOL, f"total lnl: held {total!r}, sum of the loci's {held_sum!r} (rel {e:.3e})"
    if worst is not None:
        for k, v in seen.items():
            worst[k] = max(worst.get(k, 0.0), v)
    return seen


# ---- data sets shared by tests/test_state_invariants.py and tests/test_gpu_state_invariants.py
def several_sequences_data(nloci=120):
    """the data of tests/test_gpu_sampler.py::test_several_sequences_per_species: two species with three sequences each
    -> (data, species of the tips, (parent, tau0, thetas))"""
    rng = np.random.default_rng(8)
    species = [0, 0, 0, 1, 1, 1]
    data = []
    for _ in range(nloci):
        t = sorted(rng.uniform(0.0002, 0.0028, 4))
        left = [-1] * 6 + [0, 6, 3, 8, 7]
        right = [-1] * 6 + [1, 2, 4, 5, 9]
        times = [0.0] * 6 + [t[0], t[2], t[1], t[3], 0.003 + rng.uniform(0.0005, 0.004)]
        seqs = ["".join(rng.choice(list("ACGT"), 60)) for _ in range(2)]
        seqs = [seqs[0]] * 3 + [seqs[1]] * 3
        seqs = ["".join(c if rng.random() > 0.05 else rng.choice(list("ACGT")) for c in s) for s in seqs]
        pats, w = bpp_amd.compress_site_patterns(seqs, True, True)
        data.append(dict(seqs=pats, weights=w, left=left, right=right, times=times, root=10, states=4, rate_cats=1,
                         model="jc69", rates=np.ones(1)))
    return data, species, ([2, 2, -1], [0.0, 0.0, 0.003], [0.002, 0.003, 0.004])


def moved(drv, tau0, thetas0, proposals, accepted):
    """the chain moved: taus and thetas changed, and a sane share of the proposals was accepted"""
    assert list(drv.taus()) != list(tau0), "the taus never moved"
    assert list(drv.thetas()) != list(thetas0), "the thetas never moved"
    assert proposals > 0 and 0.05 < accepted / proposals < 0.98, f"accepted {accepted} of {proposals}"
