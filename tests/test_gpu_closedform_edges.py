"""K7 on the device (csrc/kernels.hpp: pmatrix_dna_closed — K80, F81, HKY, T92, TN93, F84) at its edges, on every route that
evaluates it.  tests/test_gpu_closedform.py runs the models' moves from kappa = 2 at ordinary frequencies; here:

a. the single-locus API over tests/k7.py's EDGE_CASES x BL, one category and Gamma4 of alpha = 0.05 and 0.005 (lengths x rates
   from 0 and denormal to 4e3), against the oracle (bit-exact to the reference: tests/test_oracle_pin.py) at the bar of k7.level —
   8 ulp, or 5e-16 max(1, S), S the sum of an entry's |addends| from the exact twin — and against the properties the form has;
b. the same loci, their start trees scaled by 1e-6, 1 and 1e2, as one plan per route of the 4-state plans (k7.ROUTES);
c. (tests/test_gpu_closedform.py: the case gen-rest — F81, T92, F84 on the generic sampler);
d. every model's moves at the two ends of reflect(.., log 1e-5, log sum), generic and big-tree sampler;
e. bpa_plan_set_params on closed-form loci.

What needs no GPU — the oracle against the exact twin, the twin's properties, the seeds of d — is tests/
test_closedform_edges_host.py; what one MI355X showed is in NOTES.md, section 29."""
import time

import numpy as np
import pytest

import bpp_amd
from bpp_amd import GTree, Plan
from bpp_amd.api import PARAM_FREQS, PARAM_SUBST, branch_length
import closedform as CF
import k7
import oraclelib as O
import substedges as E
from common import rel
from invariants import check_state, oracle_locus
from test_gpu_gsampler import walk
from test_gpu_parity import build_batch, make_locus

pytestmark = pytest.mark.gpu

ENTRY = 8 * 2.0 ** -52                  # what k7.level allows an entry of size <= max(1, S), as a factor of max(1, S)


def held_to_oracle(got, model, f, q, rates, t, what, seen):
    """a device matrix [category][row][column] of length t against the oracle's, entrywise at k7.level; the exact twin's S is
    worked out only where the unscaled bar (S = 1) does not already hold -> the oracle's matrix"""
    want = O.orc_pmatrix_dna(model, np.asarray(f, float), np.asarray(q, float), rates, float(t))
    ok = k7.level(got, want, 1.0)
    for k in np.unique(np.nonzero(~ok)[0]):
        S = k7.addend_sums(model, f, q, float(t) * float(rates[k]))
        ok[k] = k7.level(got[k], want[k], S)
        seen["scaled"] = seen.get("scaled", 0) + 1
    if not ok.all():
        k, i, j = [int(x[0]) for x in np.nonzero(~ok)]
        S = k7.addend_sums(model, f, q, float(t) * float(rates[k]))
        raise AssertionError(f"{what}, t = {t!r} x rate {rates[k]!r}, entry ({i}, {j}): device {got[k, i, j]!r}, oracle {want[k, i, j]!r}: "
                             f"{k7.ulps(got[k, i, j], want[k, i, j]):.1f} ulp, {k7.distance(got[k, i, j], want[k, i, j], S[i, j]):.2f} x 2^-53 max(1, S), S = {S[i, j]:.3g}")
    u = k7.ulps(got, want)
    seen["ulps"] = max(seen.get("ulps", 0.0), float(u[u <= k7.PMAT_ULPS].max(initial=0.0)))
    seen["share"] = max(seen.get("share", 0.0), float((np.abs(got - want) / k7.PMAT_ATOL)[u > k7.PMAT_ULPS].max(initial=0.0)))
    return want


# ------------------------------------------------------------------------------------------------ a. the single-locus API
GAMMAS = {"one": None, "g4-0.05": k7.EDGE_ALPHA, "g4-0.005": k7.TINY_ALPHA}


@pytest.mark.parametrize("cats", list(GAMMAS))
@pytest.mark.parametrize("model", CF.CLOSED)
def test_k7_at_every_edge_case_and_length(model, cats):
    """Locus.update_matrices over BL on one locus per edge case of the model: every matrix level with the oracle's; rows that sum
    to 1, entries >= 0, pi_i P_ij = pi_j P_ji (T92: rows in the order of the states, k7.T92_ROW) within what the bar allows an
    entry twice over (device to oracle, oracle to the exact form); P(0) the oracle's bits; K80 at q = (1, 1): the matrix of its
    own branch — one value on the diagonal, one beside it, the diagonal 1 + 3/4 e1 of that e1"""
    t0 = time.time()
    eng = bpp_amd.Engine(0)
    alpha = GAMMAS[cats]
    R = 1 if alpha is None else 4
    rates = np.ones(1) if alpha is None else np.asarray(bpp_amd.compute_gamma_cats(alpha, alpha, 4))
    assert np.isfinite(rates).all() and (rates > 0).all()
    d0 = k7.edge_data(1)[0]
    bl = np.array(k7.BL)
    seen, branch = {}, 0
    for name, m, f, q in k7.cases_of(model):
        q6 = k7.padded(q)
        loc = make_locus(eng, 4, R, m, d0["seqs"], d0["weights"], np.array(f), q6, rates)
        loc.update_matrices(np.arange(len(bl)), bl)
        pi = np.array([float(x) for x in k7.stationary(m, f)])
        for n, t in enumerate(bl):
            got = loc.get_pmatrix(n)
            want = held_to_oracle(got, m, f, q6, rates, t, name, seen)
            if t == 0.0:
                assert (got == want).all(), (name, got, want)
            for k in range(R):
                S = np.maximum(1.0, k7.addend_sums(m, f, q6, float(t) * float(rates[k])))
                g = np.array(k7.rows_by_state(m, list(got[k])))
                bar = 2 * ENTRY * np.array(k7.rows_by_state(m, list(S)))
                assert (np.abs(g.sum(axis=1) - 1) <= bar.sum(axis=1) + 2.0 ** -52).all(), (name, t, k, g.sum(axis=1) - 1)
                assert (g >= -bar).all(), (name, t, k, g.min())
                flow = pi[:, None] * g
                assert (np.abs(flow - flow.T) <= pi[:, None] * bar + (pi[:, None] * bar).T).all(), (name, t, k, np.abs(flow - flow.T).max())
                if name == k7.K80_BRANCH:
                    off = got[k][0, 1]
                    assert all(got[k][i, j] == (got[k][0, 0] if i == j else off) for i in range(4) for j in range(4)), (t, got[k])
                    assert got[k][0, 0] == 1. + 3 / 4. * (-4 * off), (t, got[k][0, 0], off)
                    branch += 1
    print(f"[k7] {model} {cats}: {len(k7.cases_of(model))} cases x {len(bl)} lengths x {R} categories: within {seen.get('ulps', 0):.0f} ulp of the oracle, "
          f"beyond 8 ulp {seen.get('share', 0):.3f} of the absolute bar; matrices that needed S > 1: {seen.get('scaled', 0)}; {time.time() - t0:.1f} s")
    assert (branch > 0) == (model == "k80")
    eng.close()


# ------------------------------------------------------------------------------------------------ b. the batched routes
def make_loci(eng, data, scaling):
    return [CF.make_engine_loci(eng, [d], scaling)[0] for d in data]


def start_trees(data, scaling):
    return [GTree(d["left"], d["right"], d["times"], d["root"], scaling=scaling) for d in data]


def against_oracle(d, loc, gt, scaling, lnl, seen):
    """one locus after a plan's evaluation of its start tree: P-matrices level with the oracle's, CLVs (and scale counters) == the
    oracle's node update on the DEVICE's P-matrices, lnL within 1e-13 of the oracle's root sum over those CLVs
    -> (the device's P-matrices by node, the distance of lnL from the oracle's own evaluation)"""
    ol = oracle_locus(d, None, None, scaling, None)
    own = ol.full_lnl(list(d["left"]), list(d["right"]), list(d["times"]), d["root"])
    dpm = {}
    for nd in gt.branches():
        v = nd.node_index
        dpm[v] = loc.get_pmatrix(nd.pmatrix_index)
        held_to_oracle(dpm[v], d["model"], d["freqs"], d["exch"], ol.rates, branch_length(gt, nd), f"{d['case']} node {v}", seen)
    tips = len(d["seqs"])
    oc, osc = {v: ol.clv[v] for v in range(tips)}, {v: None for v in range(tips)}
    for nd in gt.postorder():
        v, l, r = nd.node_index, nd.left.node_index, nd.right.node_index
        oc[v], osc[v] = O.orc_partial(oc[l], oc[r], dpm[l], dpm[r], osc[l], osc[r], scaling, ol.order)
        got = loc.get_clv(nd.clv_index)
        assert (got == oc[v]).all(), f"{d['case']} node {v}: CLV differs from the node update of its children's buffers (max abs {np.abs(got - oc[v]).max():.3e})"
        if scaling:
            assert (loc.get_scaler(nd.scaler_index) == osc[v]).all(), f"{d['case']} node {v}: scale counters differ from the node update's"
    root = gt.root.node_index
    want = O.orc_lnl(oc[root], ol.freqs, ol.rw, ol.weights, osc[root], ol.order)
    assert np.isfinite(lnl) and rel(lnl, want) < 1e-13, (d["case"], lnl, want)
    return dpm, rel(lnl, own)


@pytest.mark.parametrize("route", list(k7.ROUTES))
def test_k7_on_every_batched_route(route):
    """One plan over every edge locus at three scales of its start tree (k7.route_data).  Which kernel a plan launches is
    plan_build's decision (csrc/engine.hip), not reported by the engine; relied on, and worked out from the loci by k7.route_of:
    every locus <= 256 patterns -> a fused plan; several categories on every locus, no scale buffers, at most 256 lanes a locus
    -> the lane-per-category kernels: the compact-record path where the loci come in the engine's slot order
    (step_s4_klane_v3_kernel where every locus has <= 16 tips, one 17-tip locus -> step_s4_klane_v2_kernel; the matrices by
    pmatrix_s4_dense_kernel), listed against it step_s4_klane_kernel<128 | 256> (the most lanes of a locus <= 128 or not); one
    category, or scale buffers -> step_s4_fused_kernel<BS, RT>, BS = 64 where the largest locus has 17 .. 64 patterns, else 256,
    RT = 1 / 4 where every locus has 1 / 4 categories, else 0; one locus of 257 patterns -> pmatrix_s4_kernel +
    partials_lnl_s4_kernel.  Asserted from the engine's timing: only the unfused path reports a P-matrix phase of its own.
    Every route's matrices are the bits of the single-locus API's for the same values: one function, pmatrix_dna_closed."""
    t0 = time.time()
    R, scaling, reverse, extra, kernel = k7.ROUTES[route]
    data = k7.route_data(route)
    n = len(data)
    assert k7.route_of(data, scaling, reverse) == kernel
    eng = bpp_amd.Engine(0)
    loci, trees = make_loci(eng, data, scaling), start_trees(data, scaling)
    order = list(reversed(range(n))) if reverse else list(range(n))
    plan = Plan(eng, [loci[k] for k in order], *build_batch([loci[k] for k in order], [trees[k] for k in order]))
    eng.enable_timing(True)
    plan.launch()
    tm = eng.timing()
    eng.enable_timing(False)
    assert tm["steps"] == 1 and (tm["pmatrix_ms"] > 0) == (route == "unfused"), tm
    lnl = plan.lnl()
    seen, far, mats = {}, 0.0, []
    for pos, k in enumerate(order):
        dpm, dist = against_oracle(data[k], loci[k], trees[k], scaling, lnl[pos], seen)
        assert np.isfinite(dist), (data[k]["case"], dist)
        far = max(far, dist)
        mats.append((k, dpm))
    plan.launch()
    assert (plan.lnl() == lnl).all()
    plan.close()
    single = make_loci(eng, data, scaling)
    for k, dpm in mats:
        gt = start_trees([data[k]], scaling)[0]
        bpp_amd.locus_update_all_matrices(single[k], gt)
        for nd in gt.branches():
            assert (single[k].get_pmatrix(nd.pmatrix_index) == dpm[nd.node_index]).all(), f"{data[k]['case']} node {nd.node_index}: not the single-locus API's bits"
    print(f"[k7] route {route} ({kernel}): {n} loci, P-matrices within {seen.get('ulps', 0):.0f} ulp of the oracle, beyond 8 ulp {seen.get('share', 0):.3f} of the "
          f"absolute bar, {seen.get('scaled', 0)} needed S > 1; lnL within {far:.2e} of the oracle's from its own P-matrices; {time.time() - t0:.1f} s")
    eng.close()


# ------------------------------------------------------------------------------------------------ d. the moves' bounds
def bound_pair(data, model, impl, seed, host=True):
    s = k7.BOUND_SHAPE
    eng = bpp_amd.Engine(0)
    hd = CF.hip_driver(eng, data, seed=seed) if host else None
    loci = CF.make_engine_loci(eng, data)
    dev = bpp_amd.Sampler(eng, loci, data, seed=seed, implementation=impl)
    if hd is not None:
        E.configure(hd, s["taxa"], s["windows"], s["R"], data, host=True)
    stree = E.configure(dev, s["taxa"], s["windows"], data=data)
    return eng, hd, dev, loci, stree


@pytest.mark.parametrize("impl", [None, "big"], ids=["generic", "big"])
@pytest.mark.parametrize("model", k7.BOUND_MODELS)
def test_moves_at_the_lower_reflection_bound(model, impl):
    """24 loci whose moved entry and one non-reference frequency start at 1.2e-5, windows of 3.0: the device sampler next to the
    host driver on the same library (seed chosen on the CPU: tests/test_closedform_edges_host.py) — identical decisions and
    counters after every iteration, lnL 1e-11, parameters 1e-11 at the end; every moved component stays >= 1e-5 (1 - 2^-52),
    some component ends an iteration inside [1e-5, 1.2e-5), some proposal is rejected; then every device buffer against a
    recompute.  K7's differences cancel at this end, so the two could part at a decision whose log-ratio differs by what the
    P-matrix bar propagates; on an MI355X none of the twelve walks did (NOTES.md, section 29)"""
    t0 = time.time()
    s = k7.BOUND_SHAPE
    data, which = k7.lower_bound_data(model)
    eng, host, dev, loci, stree = bound_pair(data, model, impl, k7.LOWER_SEEDS[model])
    assert dev.subst_steps() == CF.steps_of([model])
    hits = []

    def each(it):
        for i in range(s["nloci"]):
            f, q, _ = dev.get_subst_model(i)
            assert k7.floors_hold(model, f, q), (it, i, f, q)
            hits.extend((it, i, what) for what in k7.at_floor(model, (f, q), which[i]))

    walk(host, dev, s["iters"], s["nloci"], each=each)
    assert dev.kind() == ("big" if impl else "generic")
    for i, d in enumerate(data):
        fh, qh, ah = host.get_subst_model(i)
        fd, qd, ad = dev.get_subst_model(i)
        assert np.allclose(fd, fh, rtol=1e-11, atol=0) and np.allclose(qd, qh, rtol=1e-11, atol=0) and abs(ad - ah) <= 1e-11 * ah, i
        assert CF.untouched(model, d["exch"], qd) and max(CF.conserved(model, d["freqs"], d["exch"], fd, qd)) < 1e-12, (i, fd, qd)
    sm = dev.summary()
    print(f"[k7] lower bound {model} {dev.kind()}: {len(hits)} (iteration, locus, component) inside [1e-5, 1.2e-5): {hits[:6]}; "
          f"accepted {sm['accepted']} of {sm['proposals']}; {time.time() - t0:.1f} s")
    assert hits and 0 < sm["accepted"] < sm["proposals"]
    check_state(dev, data, stree[0], loci=loci, subst=True)
    dev.close(); host.close(); eng.close()


@pytest.mark.parametrize("impl", [None, "big"], ids=["generic", "big"])
@pytest.mark.parametrize("model", k7.BOUND_MODELS)
def test_moves_at_the_upper_reflection_bound(model, impl):
    """every locus at f = (.3, .3, .4 - 1e-9, 1e-9) with the reference entry at 1e-9: as for GTR (tests/test_gpu_subst_edges.py)
    no host trajectory is compared — v[ref] = sum - exp(l_new) cancels; after every iteration the parameters are finite and
    positive, the frequencies sum to 1 within 4 x 2^-52, the floors hold and lnL is finite; some locus leaves its start, some
    proposal is rejected, and the state is level with a recompute from the device's own parameters at the end"""
    t0 = time.time()
    s = k7.BOUND_SHAPE
    data = k7.upper_bound_data(model)
    eng, _, dev, loci, stree = bound_pair(data, model, impl, k7.UPPER_SEED, host=False)
    dev.initialize()
    assert dev.kind() == ("big" if impl else "generic")
    for it in range(s["iters"]):
        dev.iterate(1)
        for i in range(s["nloci"]):
            f, q, a = dev.get_subst_model(i)
            assert np.isfinite(f).all() and np.isfinite(q).all() and (f > 0).all() and (q > 0).all() and a > 0, (it, i, f, q, a)
            assert abs(float(f[0] + f[1] + f[2] + f[3]) - 1.0) <= 4 * 2.0 ** -52, (it, i, f, f.sum() - 1)
            assert k7.floors_hold(model, f, q), (it, i, f, q)
            assert np.isfinite(dev.tree(i)["lnl"]), (it, i)
    moved = sum(list(dev.get_subst_model(i)[k]) != list(data[i][key]) for i in range(s["nloci"]) for k, key in ((0, "freqs"), (1, "exch")))
    sm = dev.summary()
    print(f"[k7] upper bound {model} {dev.kind()}: {moved} parameter vectors of {2 * s['nloci']} left the start; accepted {sm['accepted']} of {sm['proposals']}; {time.time() - t0:.1f} s")
    assert moved > 0 and 0 < sm["accepted"] < sm["proposals"]
    check_state(dev, data, stree[0], loci=loci, subst=True)
    dev.close(); eng.close()


# ------------------------------------------------------------------------------------------------ e. bpa_plan_set_params
def test_plan_set_params_on_closed_form_loci():
    """a plan over the Gamma4 edge loci takes every locus to the NEXT case's values of its model (PARAM_FREQS, then PARAM_SUBST):
    the next launch's lnL and P-matrices are the bits of loci created at those values, and no locus's eigensystem block is
    touched (bpa_locus_get_eigen reads the same bits before and after: closed-form loci have no eigen work)"""
    data = k7.edge_data(4)
    n = len(data)
    nxt = []
    for i, d in enumerate(data):
        same = [j for j in range(n) if data[j]["model"] == d["model"]]
        nxt.append(same[(same.index(i) + 1) % len(same)])
    moved = [dict(d, freqs=data[j]["freqs"], exch=data[j]["exch"]) for d, j in zip(data, nxt)]
    assert sum((d["freqs"] != m["freqs"]).any() or (d["exch"] != m["exch"]).any() for d, m in zip(data, moved)) == n
    eng = bpp_amd.Engine(0)
    a, b = make_loci(eng, data, False), make_loci(eng, moved, False)
    ta, tb = start_trees(data, False), start_trees(moved, False)
    pa, pb = Plan(eng, a, *build_batch(a, ta)), Plan(eng, b, *build_batch(b, tb))
    pa.launch(); pb.launch()
    before = pa.lnl()
    eig = [l.get_eigen(0) for l in a]
    pa.set_params(PARAM_FREQS, np.array([m["freqs"] for m in moved]))
    pa.set_params(PARAM_SUBST, np.array([m["exch"] for m in moved]))
    pa.launch()
    la, lb = pa.lnl(), pb.lnl()
    assert (la == lb).all(), np.abs(la - lb).max()
    assert (la != before).sum() > n // 2                       # (the values did change what is computed)
    for i in range(n):
        assert all((x == y).all() for x, y in zip(a[i].get_eigen(0), eig[i])), data[i]["case"]
        for nd in ta[i].branches():
            assert (a[i].get_pmatrix(nd.pmatrix_index) == b[i].get_pmatrix(nd.pmatrix_index)).all(), (data[i]["case"], nd.node_index)
    # and the oracle at the new values
    for i in range(0, n, 7):
        m = moved[i]
        want = oracle_locus(m, None, None, False, None).full_lnl(list(m["left"]), list(m["right"]), list(m["times"]), m["root"])
        assert rel(la[i], want) < 1e-12, (m["case"], la[i], want)
    pa.close(); pb.close(); eng.close()
