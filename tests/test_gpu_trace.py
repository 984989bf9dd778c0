"""The sample trace (bpa_sampler_set_trace / _trace_read; include/bpp_amd.h): rows [iteration, lnL, taus, thetas] recorded
on the device every k iterations, on every device sampler.

A row is "what stopping there and looking would have shown": a traced sampler A and an untraced twin B start from one seed; B
stops at every row's iteration and reads taus(), thetas() and every tree's lnl.  tau and theta are compared with ==, lnL with ==
against the host replay of the documented summation order over B's per-locus values (tests/tracereplay.py), and against
summary()'s total within n 2^-53 sum|lnl_i| — the bound of a sum in any order, derived, not measured.  At the end the two
samplers hold the same state: tracing changes nothing else.
"""
import numpy as np
import pytest

import bpp_amd
import tape
import shapes
from tracereplay import replay_sum, replay_parts, any_order_bound

pytestmark = pytest.mark.gpu

# (set, moves, how): how = "v1" one launch per step (implementation="sweep"), "allreduce" a callback installed (the hybrid form)
CASES = [("persistent-4", "uniform", None), ("persistent-4", "program", None), ("persistent-mixed-tips", "program", None),
         ("persistent-4", "uniform", "v1"), ("persistent-4", "uniform", "allreduce"), ("handover-65", "program", None),
         ("generic-16-gtr-g4", "program", None), ("composite-64-65", "uniform", None), ("big-17-30", "program", None)]
KIND = {None: None, "v1": "sweep", "allreduce": "hybrid"}
TOTAL, FIRST = 30, 25


def make(eng, c, moves, how=None, seed=31, **options):
    dev = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, c["data"]), c["data"], seed=seed, implementation="sweep" if how == "v1" else None, **options)
    shapes.configure(dev, c, moves)
    if how == "allreduce":
        dev.set_allreduce(lambda p, n, st: 1, 0, 0)
    return dev


def twins(eng, c, moves, how=None, count=2):
    """samplers from one seed on one engine: every sampler's loci are made before the first is initialized (the generic sampler
    runs on the engine's packing of ALL its loci, which new loci change)"""
    devs = [make(eng, c, moves, how) for _ in range(count)]
    for d in devs:
        d.initialize()
    return devs


def parts_of(c):
    """the loci of every part of a composite, in part order (csrc/composite.hpp: the LDS kernels' JC69 loci of <= 64 patterns,
    the generic sampler's JC69 loci, its loci of several rate categories); a plain sampler: one part"""
    if c["kind"] != "composite":
        return [list(range(len(c["data"])))]
    grp = [[], [], []]
    for i, d in enumerate(c["data"]):
        grp[2 if d["rate_cats"] > 1 else 0 if len(d["weights"]) <= 64 else 1].append(i)
    assert all(len(g) for g in grp) and len(grp[0]) >= 64
    return grp


def state(dev, c):
    """everything a sampler holds that a getter shows; c["subst"], and where a case has them c["rates"], c["hered"] and
    c["gibbs"] (tests/test_gpu_trace_tails.py), say which features are on: their values and their counters are part of it"""
    s = dev.summary()
    n = len(c["data"])
    out = dict(taus=dev.taus(), thetas=dev.thetas(), trees=[dev.tree(i) for i in range(n)],
               counts=(s["proposals"], s["accepted"]))
    if c["subst"]:
        out["subst"] = [tuple(np.asarray(x).tolist() for x in dev.get_subst_model(i)) for i in range(n)]
    if c.get("rates"):
        mui, mubar = dev.get_locus_rates()
        out["rates"] = (mui.tolist(), mubar)
        out["rate_counts"] = dev.locusrate_counters()
    if c.get("hered"):
        out["hered"] = dev.get_heredity().tolist()
        out["hered_counts"] = dev.heredity_counters()
    if c.get("gibbs"):
        out["gibbs"] = tuple(dev.gibbs_counters())
    return out


def same_state(a, b):
    assert a["taus"] == b["taus"] and a["thetas"] == b["thetas"] and a["counts"] == b["counts"]
    for i, (x, y) in enumerate(zip(a["trees"], b["trees"])):
        for key in x:
            assert np.array_equal(x[key], y[key]), (i, key)
    if "subst" in a:
        assert a["subst"] == b["subst"]
    assert a.keys() == b.keys()
    for key in a.keys() - {"taus", "thetas", "counts", "trees", "subst"}:
        assert a[key] == b[key], (key, a[key], b[key])


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("name,moves,how", CASES, ids=[f"{n}-{m}" + (f"-{h}" if h else "") for n, m, h in CASES])
def test_rows_equal_stop_and_look_and_tracing_is_neutral(name, moves, how, every):
    c = shapes.case(name)
    n = len(c["data"])
    eng = bpp_amd.Engine(0)
    A, B = twins(eng, c, moves, how)
    assert A.kind() == B.kind() == (KIND[how] or c["kind"])
    npop = len(c["stree"][0])
    assert A.trace_width() == 2 + 2 * npop
    A.set_trace(every, 8 if every == 1 else 4096)           # (8: the device buffer fills up and moves to the host, three times)
    A.iterate(FIRST)
    A.iterate(TOTAL - FIRST)
    rows = A.trace()
    want_it = list(range(every, TOTAL + 1, every))
    assert rows["iteration"].dtype == np.int64 and list(rows["iteration"]) == want_it           # the count carries over between the calls
    assert rows["taus"].shape == rows["thetas"].shape == (len(want_it), npop) and rows["lnl"].shape == (len(want_it),)
    parts = parts_of(c)
    done = 0
    for r, it in enumerate(want_it):
        B.iterate(it - done)
        done = it
        assert list(rows["taus"][r]) == B.taus() and list(rows["thetas"][r]) == B.thetas(), it
        lnl = np.array([B.tree(i)["lnl"] for i in range(n)])
        replay = replay_parts([lnl[p] for p in parts])
        total = B.summary()["total_lnl"]
        print(f"[trace] {name} {moves} {how} every {every} it {it}: row {rows['lnl'][r]!r} replay {replay!r} summary {total!r} bound {any_order_bound(lnl):.3g}")
        assert rows["lnl"][r] == replay, it
        assert abs(rows["lnl"][r] - total) <= any_order_bound(lnl), it
    if done < TOTAL:
        B.iterate(TOTAL - done)
    assert rows["taus"][-1].tolist() != list(c["stree"][1]) and len(set(rows["lnl"])) > 1          # the chain moved
    assert len(A.trace()["lnl"]) == 0
    same_state(state(A, c), state(B, c))
    A.close(); B.close(); eng.close()


def _program4(eng, every, capacity, seed=31, **options):
    c = shapes.case("persistent-4")
    dev = make(eng, c, "program", seed=seed, **options)
    dev.initialize()
    assert dev.kind() == "persistent"
    if every is not None:
        dev.set_trace(every, capacity)
    return dev, c


def test_capacity_and_draining():
    eng = bpp_amd.Engine(0)
    X, c = _program4(eng, 1, 64)
    Y, _ = _program4(eng, 1, 4)
    X.iterate(40); Y.iterate(40)
    w = 2 + 2 * len(c["stree"][0])
    assert X.trace_width() == Y.trace_width() == w
    big = X.trace_read()
    assert big.shape == (40, w) and list(big[:, 0]) == list(range(1, 41))
    r1 = Y.trace_read(10)
    r2 = Y.trace_read()
    assert r1.shape == (10, w) and r2.shape == (30, w)
    assert np.array_equal(np.concatenate([r1, r2]), big)             # the oldest first, each once, the same bits at either capacity
    assert len(Y.trace()["iteration"]) == 0 and len(X.trace()["iteration"]) == 0
    same_state(state(X, c), state(Y, c))
    X.close(); Y.close(); eng.close()


def test_a_launch_that_gives_up_writes_no_row_and_the_rerun_writes_them_in_order(capfd):
    """inject=2 (as tests/test_gpu_sampler.py uses it): the second persistent launch returns at its first wait and
    leaves the loci as it found them; the launches behind it give up at once.  With every = 2 a launch is two iterations, so
    iterate(6) + iterate(4) is five launches, of which four do not run — nor may their rows be written; reading the trace
    runs them again."""
    eng = bpp_amd.Engine(0)
    P, c = _program4(eng, 2, 16)
    Q, _ = _program4(eng, 2, 16, inject=2)
    for dev in (P, Q):
        dev.iterate(6); dev.iterate(4)
    capfd.readouterr()
    want = P.trace_read()
    assert "run again" not in capfd.readouterr().err
    got = Q.trace_read()
    assert "8 iterations are run again" in capfd.readouterr().err
    assert list(want[:, 0]) == [2, 4, 6, 8, 10] and np.array_equal(got, want)
    same_state(state(P, c), state(Q, c))
    P.close(); Q.close(); eng.close()


def test_burnin_writes_no_rows_and_the_trace_can_be_switched_off():
    eng = bpp_amd.Engine(0)
    dev, c = _program4(eng, 1, 16)
    ref, _ = _program4(eng, None, 0)
    dev.burnin(40); ref.burnin(40)
    assert len(dev.trace()["iteration"]) == 0
    dev.iterate(3); ref.iterate(3)
    rows = dev.trace()
    assert list(rows["iteration"]) == [1, 2, 3]
    assert list(rows["taus"][-1]) == ref.taus() and list(rows["thetas"][-1]) == ref.thetas()
    dev.set_trace(0, 0)
    dev.iterate(3); ref.iterate(3)
    assert len(dev.trace()["iteration"]) == 0
    with pytest.raises(bpp_amd.BpaError, match="capacity"):
        dev.set_trace(1, 0)
    same_state(state(dev, c), state(ref, c))
    dev.close(); ref.close()
    eng.set_options(usedata=0, bfbeta=1.0)
    try:
        dev, c = _program4(eng, 1, 16)
        dev.iterate(3)
        rows = dev.trace()
        assert list(rows["iteration"]) == [1, 2, 3] and list(rows["lnl"]) == [0.0, 0.0, 0.0]
        assert list(rows["taus"][-1]) == dev.taus() and rows["taus"][-1].tolist() != list(c["stree"][1])
        dev.close()
    finally:
        eng.set_options(usedata=1, bfbeta=1.0)
    eng.close()
