"""Every code path that takes `scaling=True`, on loci whose scale counters are NOT zero (tests/firing.py; the same sets on the
CPU, with the reference-API host driver: tests/test_scaling_fires.py).  The other tests that pass scaling=True compare counters
that all stay 0.  Each test here first proves from the ORACLE's recompute — never from a device buffer — that its input fires
(firing.fires_at_start: per locus two inner nodes or more with a counter, one of them below the root; over the set a node with
zero and non-zero counters side by side and a counter >= 2), and at every later checkpoint that it still does
(firing.still_fires).  Bars: the project's own — integers and CLVs ==, lnL 1e-13 (plans, tape steps) / 1e-12 (from-scratch
recompute, check_state), P-matrices 8 ulp or 5e-16.

Which test reaches which scaling kernel with non-zero counters (engine.hip: plan_build / plan_launch_mode decide):
  step_jc69_v2_kernel              test_plan_routes[jc69-packed*], tapes, host driver (JC69, one category, every locus < 256 patterns
                                   and listed in the engine's slot order: plan_build sets jc69_v2)
  step_jc69_v2_chain_kernel        test_chain_of_two_plans..., test_chain_launch_equals_step_by_step_where_counters_fire
  step_jc69_kernel<64 | 256>       test_plan_routes[jc69-unpacked*] (the same loci listed against the slot order: jc69_v2 stays off,
                                   fused_jc69 holds; workgroup 64 where the largest locus has 17 .. 64 patterns, else 256)
  step_s4_fused_kernel<64 | 256, 1 | 0 | 4>   test_plan_routes[gtr-*] (a locus with scale buffers keeps the batch off the lane-per-category
                                   kernels; fused_rt = 1 / 4 where every locus has 1 / 4 categories, else 0), the GTR tape
  partials_lnl_wave20_kernel, _pipemfma20_, _tiled_   test_20_state_kernels_where_counters_fire (BPA_S20_KERNEL unset, pipemfma, tiled)
  partials_lnl_s4_kernel, and the sampler's toggling of scale-buffer indices   test_big_tree_sampler_where_counters_fire
  the C host driver's `scaling`    test_same_trajectory_on_gpu_and_reference_where_counters_fire
"""
import os

import numpy as np
import pytest

import bpp_amd
from bpp_amd import GTree, Plan, OP_DTYPE
import oraclelib as O
import hostdrv
import shapes
import tape
import firing
from common import rel
from invariants import check_state, moved, oracle_locus, ulps, PMAT_ULPS, PMAT_ATOL
from test_gpu_parity import build_batch, full_eval, LNL_RTOL_TIGHT
from test_gpu_gsampler import walk

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ 1. batched plans
def start_trees(data, scaling):
    return [GTree(d["left"], d["right"], d["times"], d["root"], scaling=s) for d, s in zip(data, scaling)]


def held(loc, gt, scaling):
    """every inner node's CLV and scale buffer, as the device holds them"""
    return ({nd.node_index: loc.get_clv(nd.clv_index) for nd in gt.postorder()},
            {nd.node_index: loc.get_scaler(nd.scaler_index) for nd in gt.postorder()} if scaling else {})


def against_oracle(i, d, loc, gt, scaling, lnl):
    """locus i after an evaluation of its start tree: lnL, P-matrices, scale buffers and CLVs against the oracle (the CLVs against
    the oracle's node update on the DEVICE's P-matrices, as invariants.check_state step 9) -> (CLVs, scale buffers)"""
    ol = oracle_locus(d, None, None, scaling, None)
    want = ol.full_lnl(list(d["left"]), list(d["right"]), list(d["times"]), d["root"])
    assert np.isfinite(want), (i, want)
    dpm = {}
    for nd in gt.branches():
        v = nd.node_index
        dpm[v] = loc.get_pmatrix(nd.pmatrix_index)
        u, a = ulps(dpm[v], ol.pmat[v]).max(), np.abs(dpm[v] - ol.pmat[v]).max()
        assert u <= PMAT_ULPS or a < PMAT_ATOL, f"locus {i} node {v} P-matrix: {u:.1f} ulp, {a:.3e} absolute"
    clv, sc = held(loc, gt, scaling)
    tips = len(d["seqs"])
    oc, osc = {v: ol.clv[v] for v in range(tips)}, {v: None for v in range(tips)}
    for nd in gt.postorder():
        v, l, r = nd.node_index, nd.left.node_index, nd.right.node_index
        oc[v], osc[v] = O.orc_partial(oc[l], oc[r], dpm[l], dpm[r], osc[l], osc[r], scaling, ol.order)
        if scaling:
            assert (sc[v] == ol.scaler[v]).all(), f"locus {i} node {v}: scale buffer differs from the oracle's"
            assert (sc[v] == osc[v]).all(), f"locus {i} node {v}: scale buffer differs from the node update's counters"
        assert (clv[v] == oc[v]).all(), f"locus {i} node {v}: CLV differs from the node update of its children's buffers (max abs {np.abs(clv[v] - oc[v]).max():.3e})"
    print(f"[fires] locus {i}: lnl {lnl!r} oracle {want!r} rel {rel(lnl, want):.2e}")
    assert rel(lnl, want) < LNL_RTOL_TIGHT, (i, lnl, want)
    return clv, sc


def evaluate_as_plan(eng, c, scaling=None, reverse=False):
    """the set's start trees as ONE plan on a fresh engine's loci -> per locus (lnL, CLVs, scale buffers), every one checked
    against the oracle and against the single-locus path on a second set of loci (same bits).  scaling: per locus (default: all
    with scale buffers); reverse: the loci listed against the engine's slot order"""
    data = c["data"]
    n = len(data)
    scaling = [True] * n if scaling is None else list(scaling)
    loci = [tape.make_engine_loci(eng, [d], s)[0] for d, s in zip(data, scaling)]
    trees = start_trees(data, scaling)
    order = list(reversed(range(n))) if reverse else list(range(n))
    plan = Plan(eng, [loci[k] for k in order], *build_batch([loci[k] for k in order], [trees[k] for k in order]))
    plan.launch()
    got = plan.lnl()
    out = [None] * n
    for pos, k in enumerate(order):
        out[k] = (got[pos],) + against_oracle(k, data[k], loci[k], trees[k], scaling[k], got[pos])
    plan.launch()                                                   # (idempotent)
    assert (plan.lnl() == got).all()
    plan.close()
    single = [tape.make_engine_loci(eng, [d], s)[0] for d, s in zip(data, scaling)]
    for k in range(n):
        t2 = start_trees([data[k]], [scaling[k]])[0]
        assert full_eval(single[k], t2) == out[k][0], k
        clv, sc = held(single[k], t2, scaling[k])
        assert all((clv[v] == out[k][1][v]).all() for v in clv) and all((sc[v] == out[k][2][v]).all() for v in sc), k
    return out


ROUTES = {  # name -> (set, reverse, every other locus without scale buffers)
    "jc69-packed-5": ("plan-jc69-1-5", False, False), "jc69-packed-3": ("plan-jc69-1-3", False, False),
    "jc69-unpacked-256": ("plan-jc69-1-5", True, False), "jc69-unpacked-64": ("plan-jc69-1-3", True, False),
    "gtr-1cat-256": ("plan-gtr-1-5", False, False), "gtr-1cat-64": ("plan-gtr-1-3", False, False),
    "gtr-3cat-256": ("plan-gtr-3-5", False, False), "gtr-3cat-64": ("plan-gtr-3-3", False, False),
    "gtr-4cat-256": ("plan-gtr-4-5", False, False), "gtr-4cat-64": ("plan-gtr-4-3", False, False),
    "jc69-mixed": ("plan-jc69-1-5", False, True), "gtr-4cat-mixed": ("plan-gtr-4-5", False, True),
}


@pytest.mark.parametrize("route", list(ROUTES))
def test_plan_routes_where_counters_fire(route):
    """One batch of firing 24-tip loci (f = 1e-6; 1, 63, 64, 65 and 193 patterns, or 1, 63, 64) per route of the 4-state
    plans; relied on, from engine.hip's plan_build: every locus has <= 256 patterns, so the plan is a fused one; JC69 with one
    category and the loci in slot order -> step_jc69_v2_kernel; the same loci in reverse order -> step_jc69_kernel<BS>; any
    other model with a locus that has scale buffers -> step_s4_fused_kernel<BS, RT> with RT = 1, 4 (every locus 1 / 4
    categories) or 0 (three), and BS = 64 where the largest locus has 17 .. 64 patterns, else 256.  `mixed`: every other
    locus has no scale buffers (its lnL is finite without: the oracle says so)."""
    name, reverse, mixed = ROUTES[route]
    c = firing.case(name)
    firing.fires_at_start(c["data"])
    big = max(len(d["weights"]) for d in c["data"])
    assert (big == 64) == route.endswith(("-64", "-3")) and big <= 256
    eng = bpp_amd.Engine(0)
    out = evaluate_as_plan(eng, c, [k % 2 == 0 for k in range(len(c["data"]))] if mixed else None, reverse)
    assert all(np.isfinite(o[0]) for o in out)
    if mixed:
        assert any(s.any() for o in out[::2] for s in o[2].values()) and not any(o[2] for o in out[1::2])
    eng.close()


def test_chain_of_two_plans_reads_the_counters_the_first_has_just_written():
    """bpa_plans_launch on two plans over the firing JC69 loci as ONE launch (step_jc69_v2_chain_kernel): the first evaluates the
    start trees, the second updates every root again into the OTHER half of its buffer pair from the children's CLVs and counters
    the first has written in the same launch.  Both halves then hold the oracle's root, and the second plan's lnL the first's bits"""
    c = firing.case("plan-jc69-1-5")
    data = c["data"]
    firing.fires_at_start(data)
    eng = bpp_amd.Engine(0)
    loci = tape.make_engine_loci(eng, data, True)
    trees = start_trees(data, [True] * len(data))
    first = Plan(eng, loci, *build_batch(loci, trees))
    zeros = np.zeros(len(data) + 1, dtype=np.uint32)
    ops, roots = [], []
    for gt in trees:
        inner = gt.inner_count
        a = list(bpp_amd.api.node_op(gt.root))
        a[0], a[1] = a[0] + inner, a[1] + inner
        ops.append(tuple(a)); roots.append((a[0], a[1]))
    second = Plan(eng, loci, zeros, np.zeros(0, dtype=np.uint32), np.zeros(0), np.arange(len(data) + 1, dtype=np.uint32),
                  np.array(ops, dtype=OP_DTYPE), np.array([r[0] for r in roots], dtype=np.uint32), np.array([r[1] for r in roots], dtype=np.int32))
    eng.enable_timing(True)
    bpp_amd.PlanSequence([first, second]).launch()
    tm = eng.timing()
    eng.enable_timing(False)
    assert tm["steps"] == 2 and tm["launches"] == 1, tm
    a, b = first.lnl(), second.lnl()
    assert (a == b).all(), (a, b)
    for i, (d, loc, gt) in enumerate(zip(data, loci, trees)):
        against_oracle(i, d, loc, gt, True, a[i])
        assert (loc.get_clv(roots[i][0]) == loc.get_clv(gt.root.clv_index)).all(), i
        assert (loc.get_scaler(roots[i][1]) == loc.get_scaler(gt.root.scaler_index)).all() and loc.get_scaler(roots[i][1]).any(), i
    first.close(); second.close(); eng.close()


@pytest.mark.parametrize("R", [1, 4])
def test_20_state_kernels_where_counters_fire(R, monkeypatch):
    """LG loci of 16 tips at f = 1e-4 (1, 63, 64, 65, 193 patterns) and one of 24 tips (65 patterns: the set's counter >= 2) as one
    plan on the default 20-state kernel, on pipemfma and on tiled (BPA_S20_KERNEL is read when a plan is built): each against the
    oracle, and the three bit for bit against each other — lnL, CLVs and counters"""
    c = firing.case(f"plan-lg-{R}-5")
    firing.fires_at_start(c["data"])
    runs = {}
    for kernel in (None, "pipemfma", "tiled"):
        if kernel is None:
            monkeypatch.delenv("BPA_S20_KERNEL", raising=False)
        else:
            monkeypatch.setenv("BPA_S20_KERNEL", kernel)
        eng = bpp_amd.Engine(0)
        runs[kernel] = evaluate_as_plan(eng, c)
        eng.close()
    monkeypatch.delenv("BPA_S20_KERNEL", raising=False)
    base = runs[None]
    for kernel in ("pipemfma", "tiled"):
        for k, (x, y) in enumerate(zip(base, runs[kernel])):
            assert x[0] == y[0], (kernel, k, x[0], y[0])
            assert all((x[1][v] == y[1][v]).all() for v in x[1]) and all((x[2][v] == y[2][v]).all() for v in x[2]), (kernel, k)


# ------------------------------------------------------------------ 2. tapes
@pytest.mark.parametrize("name", ["tape-jc69", "tape-gtr-g4"])
def test_tape_gpu_vs_oracle_where_counters_fire(name):
    """tests/test_gpu_tape.py::test_tape_gpu_vs_oracle's scheme on four firing 24-tip loci (30, 65, 1 and 64 patterns): 3 A00
    iterations, every step's lnL against the oracle's replay at 1e-13, the final trees from scratch at 1e-12"""
    c = firing.case(name)
    data = c["data"]
    firing.fires_at_start(data)
    eng = bpp_amd.Engine(0)
    loci = tape.make_engine_loci(eng, data, True)
    sch, steps = firing.tape_steps(c)
    firing.still_fires(data, sch.trees)
    got = []
    for st in steps:
        p = tape.plan_for_step(eng, loci, st)
        if st.global_decision is not None:
            if len(got) % 2:
                p.enable_sum()
            else:
                assert p.enable_partial_sums() >= 1
        p.launch()
        lnl = p.lnl()
        if st.global_decision is not None:
            assert rel(p.lnl_sum(), float(np.sum(lnl))) < 1e-13
        got.append(lnl)
        p.close()
    worst = 0.0
    for li, d in enumerate(data):
        sub = tape.locus_subtape(steps, li)
        want = tape.oracle_replay(d, sub, True)
        mine = np.array([got[s["step"]][s["task"]] for s in sub])
        worst = max(worst, float(np.max(np.abs(mine - want) / np.abs(want))))
        print(f"[fires] {name} locus {li}: {len(sub)} steps, largest relative difference {np.max(np.abs(mine - want) / np.abs(want)):.2e}")
        assert np.all(np.abs(mine - want) <= 1e-13 * np.abs(want)), (li, np.max(np.abs(mine - want) / np.abs(want)))
    for li, d in enumerate(data):
        tr = sch.trees[li]
        want = oracle_locus(d, None, None, True, None).full_lnl(tr.left, tr.right, tr.time, tr.root)
        have = loci[li].root_loglikelihood(tr.clv[tr.root], tr.scaler[tr.root])
        assert rel(have, want) < 1e-12, (li, have, want)
    print(f"[fires] {name}: {len(steps)} steps, largest relative difference {worst:.2e}; (nodes, top) at the start {firing.summary(data)}, at the end {firing.summary(data, sch.trees)}")
    eng.close()


def test_chain_launch_equals_step_by_step_where_counters_fire():
    """tests/test_gpu_tape.py::test_chain_launch_equals_step_by_step's scheme on the firing JC69 set: every step's lnL, and EVERY
    locus's CLVs, scale buffers and P-matrices left behind, are the bits of the launches one by one"""
    c = firing.case("tape-jc69")
    data = c["data"]
    firing.fires_at_start(data)
    sch, steps = firing.tape_steps(c, seed=9, iterations=2)
    firing.still_fires(data, sch.trees)
    runs = []
    for chained in (False, True):
        eng = bpp_amd.Engine(0)
        loci = tape.make_engine_loci(eng, data, True)
        plans = []
        for st in steps:
            p = tape.plan_for_step(eng, loci, st)
            if st.global_decision is not None:
                p.enable_partial_sums()
            plans.append(p)
        if chained:
            eng.enable_timing(True)
            bpp_amd.PlanSequence(plans).launch()
            tm = eng.timing()
            eng.enable_timing(False)
            # every step accounted for, and sent out in chains (of up to BPA_CHAIN_MAX = 24 links: 147 steps are 7 launches or a few more)
            assert tm["steps"] == len(steps) and tm["launches"] <= len(steps) // 4, tm
        else:
            for p in plans:
                p.launch()
        lnl = [p.lnl() for p in plans]
        sums = [p.lnl_sum() for st, p in zip(steps, plans) if st.global_decision is not None]
        bufs = []
        for li, d in enumerate(data):
            tips = len(d["seqs"])
            tr = sch.trees[li]
            bufs.append(([loci[li].get_clv(tips + k) for k in range(2 * (tips - 1))], [loci[li].get_pmatrix(k) for k in range(2 * (2 * tips - 2))],
                         [loci[li].get_scaler(k) for k in range(2 * (tips - 1))], loci[li].root_loglikelihood(tr.clv[tr.root], tr.scaler[tr.root])))
        runs.append((lnl, bufs, sums))
        for p in plans:
            p.close()
        eng.close()
    a, b = runs
    assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0]))
    for li, (x, y) in enumerate(zip(a[1], b[1])):
        for part in range(3):
            assert all(np.array_equal(u, v) for u, v in zip(x[part], y[part])), (li, part)
        assert x[3] == y[3], li
        assert any(s.any() for s in x[2]), li
    assert len(a[2]) > 0 and a[2] == b[2]


# ------------------------------------------------------------------ 3. the C host driver on the library against the reference's locus API
@pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref did not travel")
@pytest.mark.parametrize("name", ["big-24", "big-24-gtr-g4"])
def test_same_trajectory_on_gpu_and_reference_where_counters_fire(name):
    """tests/test_gpu_host_driver.py::test_same_trajectory_on_gpu_and_reference on six firing 24-tip loci: identical decisions,
    identical trees and buffer indices, lnL to 1e-12"""
    c = firing.case(name)
    data = c["data"]
    n = len(data)
    firing.fires_at_start(data)
    eng = bpp_amd.Engine(0)
    loci = tape.make_engine_loci(eng, data, True)
    g = hostdrv.hip_driver(eng, loci, data, seed=11, scaling=True)
    r = hostdrv.reference_driver(data, seed=11, scaling=True)
    for drv in (g, r):
        shapes.configure(drv, c, "uniform", host=True)
    g.initialize(); r.initialize()
    assert rel(g.total_lnl(), r.total_lnl()) < 1e-13
    for it in range(5):
        g.iterate(); r.iterate()
        print(f"[fires] {name} iteration {it}: total lnl rel {rel(g.total_lnl(), r.total_lnl()):.2e}")
        assert rel(g.total_lnl(), r.total_lnl()) < 1e-12, it
        assert g.counters() == r.counters(), it
    assert g.taus() == r.taus() and g.taus() != list(c["stree"][1])
    props, acc, _ = g.counters()
    assert 0.05 < acc / props < 0.98
    for i in range(n):
        a, b = g.tree(i), r.tree(i)
        for key in ("root", "left", "right", "parent", "clv", "pmat", "scaler", "pop"):
            assert a[key] == b[key], (i, key)
        assert a["time"] == b["time"] and a["logpr"] == b["logpr"]
        assert rel(a["lnl"], b["lnl"]) < 1e-12
    firing.still_fires(data, [r.tree(i) for i in range(n)])
    g.close(); r.close(); eng.close()


# ------------------------------------------------------------------ 4. the big-tree sampler
SAMPLER_SETS = ["big-17", "big-24", "big-24-gtr-g4", "big-64"]
WORST = {}


def sampler(eng, c, moves, seed):
    loci = tape.make_engine_loci(eng, c["data"], True)
    dev = bpp_amd.Sampler(eng, loci, c["data"], seed=seed)
    shapes.configure(dev, c, moves)
    return dev, loci


def grow_where_counters_fire(name, moves, eng, chunks=(1, 3, 30)):
    """a fresh sampler on the set, iterated to each count of `chunks`: check_state (every scale buffer and CLV ==, the root term
    through the root's scale buffer) and firing.still_fires after each -> (sampler, loci); the chain moved inside moved()'s band"""
    c = firing.case(name)
    data, (parent, tau0, thetas0) = c["data"], c["stree"]
    n = len(data)
    dev, loci = sampler(eng, c, moves, 31)
    dev.initialize()
    assert dev.kind() == "big"
    worst = WORST.setdefault((name, moves), {})
    check_state(dev, data, parent, tip_species=c["species"], scaling=True, loci=loci, worst=worst)
    line, done = [firing.summary(data)], 0
    for upto in chunks:
        dev.iterate(upto - done)
        done = upto
        check_state(dev, data, parent, tip_species=c["species"], scaling=True, loci=loci, worst=worst)
        trees = [dev.tree(i) for i in range(n)]
        firing.still_fires(data, trees)
        line.append(firing.summary(data, trees))
    s = dev.summary()
    moved(dev, tau0, thetas0, s["proposals"], s["accepted"])
    print(f"[fires] {name} {moves}: {done} iterations, accepted {s['accepted'] / s['proposals']:.2f}: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items()))
          + "; nodes with a counter per locus at " + " / ".join(f"{k}: {[x[0] for x in v]}" for k, v in zip((0,) + tuple(chunks), line))
          + f"; largest counter {[max(x[1] for x in v) for v in line]}")
    return dev, loci


@pytest.mark.parametrize("moves", ["uniform", "program"])
@pytest.mark.parametrize("name", SAMPLER_SETS)
def test_big_tree_sampler_where_counters_fire(name, moves):
    """17 (+ three 24-tip loci, see firing.py), 24 and 64 tips under JC69, 24 tips under GTR + Gamma4: (a) the device walks the C
    host driver's trajectory on the same library for 4 iterations (walk() and its tolerances: tests/test_gpu_sampler_limits.py),
    trees and population labels equal; (b) a fresh sampler's whole state against the CPU recompute after 1, 3 and 30 iterations"""
    c = firing.case(name)
    data = c["data"]
    n = len(data)
    firing.fires_at_start(data)
    eng = bpp_amd.Engine(0)
    host = hostdrv.hip_driver(eng, tape.make_engine_loci(eng, data, True), data, seed=29, scaling=True)
    shapes.configure(host, c, moves, host=True)
    dev, _ = sampler(eng, c, moves, 29)
    walk(host, dev, 4, n, **(dict(tol=1e-9) if moves == "program" else {}))
    assert dev.kind() == "big"
    firing.still_fires(data, [host.tree(i) for i in range(n)])
    host.close(); dev.close()
    dev, _ = grow_where_counters_fire(name, moves, eng)
    dev.close(); eng.close()


# ------------------------------------------------------------------ 5. the checker sees what it should
@pytest.fixture(scope="module")
def grown():
    """the state test 4 (b) leaves behind on the 24-tip JC69 set"""
    eng = bpp_amd.Engine(0)
    dev, loci = grow_where_counters_fire("big-24", "uniform", eng)
    c = firing.case("big-24")
    yield dev, loci, c, dict(data=c["data"], species_parent=c["stree"][0], tip_species=c["species"], scaling=True, loci=loci)
    dev.close(); eng.close()


def _firing_node(dev, loci, c, root):
    """(locus, node, its scale buffer's index) of a node with a non-zero counter ON THE ORACLE's recompute: the root, or a node below"""
    n = len(c["data"])
    for i, (lnl, sc, rt) in enumerate(firing.counters(c["data"], [dev.tree(k) for k in range(n)])):
        for v, s in sc.items():
            if s.any() and (v == rt) == root:
                return i, v, int(dev.tree(i)["clv"][v]) - len(c["data"][i]["seqs"])
    raise AssertionError("no such node")


def test_the_grown_state_passes(grown):
    dev, loci, c, kw = grown
    check_state(dev, **kw)


@pytest.mark.parametrize("root", [False, True])
def test_checker_sees_one_counter_off_by_one(grown, root):
    """bpa_locus_set_scaler writes one counter + 1 into a firing node's scale buffer (test-owned, written back afterwards): below
    the root check_state names that scale buffer, at the root the root buffer's lnL (off by one log 2^-256 times the weight)"""
    dev, loci, c, kw = grown
    i, v, idx = _firing_node(dev, loci, c, root)
    was = loci[i].get_scaler(idx)
    bad = was.copy()
    bad[int(np.argmax(was))] += 1
    loci[i].set_scaler(idx, bad)
    try:
        with pytest.raises(AssertionError, match=rf"locus {i} root buffer" if root else rf"locus {i} node {v} scale buffer {idx}"):
            check_state(dev, **kw)
    finally:
        loci[i].set_scaler(idx, was)
    check_state(dev, **kw)


class Pointed:
    """a sampler whose tree(i) names, for node v, the OTHER half of the node's buffer pair (clv - tips +- inner)"""

    def __init__(self, dev, i, v, tips):
        self.dev, self.i, self.v, self.tips = dev, i, v, tips

    def __getattr__(self, name):
        return getattr(self.dev, name)

    def tree(self, k):
        t = self.dev.tree(k)
        if k == self.i:
            inner = self.tips - 1
            t["clv"][self.v] = self.tips + (int(t["clv"][self.v]) - self.tips + inner) % (2 * inner)
        return t


@pytest.mark.parametrize("root", [False, True])
def test_checker_sees_the_other_half_of_a_toggled_pair(grown, root):
    """the index pair of a firing node read the wrong way round: the other half holds what a rejected proposal or an earlier
    state left there (or nothing yet)"""
    dev, loci, c, kw = grown
    i, v, _ = _firing_node(dev, loci, c, root)
    with pytest.raises(AssertionError, match=rf"locus {i} (root buffer|node \d+ (CLV|scale) buffer)"):
        check_state(Pointed(dev, i, v, len(c["data"][i]["seqs"])), **kw)
