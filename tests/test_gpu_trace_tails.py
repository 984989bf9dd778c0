"""The sample trace (bpa_sampler_set_trace / _trace_read; include/bpp_amd.h) where tests/test_gpu_trace.py does not reach:

 A. under the moves that follow MIX in an iteration — HRDT, the nine substitution-parameter steps, MUI (left pending when the
    rates' mean is fixed), MUBAR — on the generic and on the big-tree sampler, and under the inverse-gamma priors; the row is
    written behind the settle of whichever step closed the iteration (gs_iterate, either sampler's: the extra step of mode 4);
 B. on more loci than trace_row_kernel has threads (1 025 and 2 500: the second and third trip of its loop);
 C. the buffer hand-over, partial reads, the burn-in's hold and a second set_trace off the persistent kernel: on the generic
    sampler (part-batches on several streams), the big-tree sampler and a composite (the merge of the parts' rows).

Every case runs THREE samplers from one seed: A is traced, B is untraced and stops at every row's iteration (a row is what
stopping there and looking shows), C is untraced and runs all its iterations in ONE call — a row's iteration is the only place
where the traced chain does something the plain one does not, and B does something there too (a getter settles and downloads).
Comparisons are == throughout, or the any-order bound n 2^-53 sum|lnl_i| of tests/tracereplay.py against summary()'s total."""
import numpy as np
import pytest

import bpp_amd
from bpp_amd import synth
import heredity as HD
import invariants
import invgamma as IG
import locusrates as LR
import shapes
import tape
from tracereplay import replay_sum, replay_parts, any_order_bound
from test_gpu_trace import twins, parts_of, state, same_state
from test_gpu_bigsampler_subst import set17, moved_components
from test_gpu_invgamma import gtr8, SP8

pytestmark = pytest.mark.gpu

SEED = 31
TOTAL, FIRST = 30, 25


# ------------------------------------------------------------------ A. rows under the tails
def _set(name):
    """-> (the dict locusrates.configure / shapes.configure takes, the sampler's options)"""
    if name == "b12":
        return LR.case("b", 12), {}
    if name == "b12-big":
        return LR.case("b", 12), dict(implementation="big")
    if name == "d8":
        return LR.case("d", 8), {}
    if name == "set17":
        return set17(4), {}
    if name == "gtr8":
        return dict(data=gtr8(6), species=[SP8]*6, stree=synth.species_tree_arrays(4), model="gtr"), {}
    if name == "jc8-sweep":
        return dict(data=synth.make_dataset(8, 300, 4, "jc69", 1, seed=47), species=None, stree=synth.species_tree_arrays(4), model="jc69"), dict(implementation="sweep")
    return shapes.case(name), {}


def _invgamma(dev, c, moves, name):
    """the inverse-gamma settings of tests/test_gpu_invgamma.py's trajectory tests on these sets"""
    program = moves == "program"
    if name == "gtr8":
        IG.configure(dev, c["stree"], c["species"], moves, theta_prior=(3.0, 0.004, 0.0004 if program else 0.001),
                     finetune=(0.003, 0.005, 0.0004, 0.05) if program else (0.003, 0.005, 0.0008, 0.2))
    elif name == "jc8-sweep":
        IG.configure(dev, c["stree"], None, moves)
    else:
        IG.configure(dev, c["stree"], c["species"], moves, theta_prior=(3.0, 0.004, 0.001), finetune=c["finetune"])


# tail -> (what is on: subst, rates, mubar, hered, gibbs)
TAIL = {"whole": dict(subst=True, rates=True, mubar=True, hered=True), "mui-pending": dict(rates=True), "hrdt": dict(hered=True),
        "subst": dict(subst=True), "mui-mubar": dict(rates=True, mubar=True), "none": {}, "invgamma": dict(gibbs=True)}


def configure(dev, c, moves, tail, name):
    n = len(c["data"])
    if tail == "whole":
        HD.configure(dev, c, moves, False, subst=True, rates=True, scalars=HD.start_scalars(n))
    elif tail == "mui-pending":                  # mu_bar fixed: MUI's evaluation closes the iteration
        LR.configure(dev, c, moves, False, mubar_prior=None, rates=LR.spread_rates(n, 0.5, 2.0))
    elif tail == "hrdt":
        HD.configure(dev, c, moves, False, scalars=HD.start_scalars(n))
    elif tail == "subst":                        # the alpha step's evaluation closes the iteration
        LR.configure(dev, c, moves, False, subst=True, ft=None)
    elif tail == "mui-mubar":
        LR.configure(dev, c, moves, False, rates=LR.spread_rates(n, 0.5, 2.0))
    elif tail == "invgamma":
        _invgamma(dev, c, moves, name)
    else:
        shapes.configure(dev, c, moves)


def recompute(dev, c, loci, tail):
    """the CPU recompute of everything the sampler holds, for the features that are on, the loci's device buffers included"""
    data, parent, on = c["data"], c["stree"][0], TAIL[tail]
    kw = dict(loci=loci, tip_species=c["species"])
    if on.get("subst"):
        kw["subst"] = True
    if on.get("hered"):
        return HD.check_state(dev, data, parent, rated=bool(on.get("rates") or on.get("subst")), **kw)
    if on.get("rates") or on.get("subst"):
        return LR.check_state(dev, data, parent, **kw)
    return invariants.check_state(dev, data, parent, **kw)


def three(eng, c, moves, tail, name, options):
    """A, B, C from one seed, each on its own engine loci: all loci are made before the first initialize (the generic sampler
    runs on the engine's packing of ALL its loci) -> the samplers, A's loci"""
    devs, loci = [], []
    for _ in range(3):
        loci.append(tape.make_engine_loci(eng, c["data"]))
        devs.append(bpp_amd.Sampler(eng, loci[-1], c["data"], seed=SEED, **options))
        configure(devs[-1], c, moves, tail, name)
    for d in devs:
        d.initialize()
    return devs, loci[0]


def tail_reading(dev, c):
    """what the tail's moves have accepted and left so far, by move"""
    n = len(c["data"])
    out = {}
    if c["hered"]:
        out["hrdt"] = dev.heredity_counters()[1]
    if c["rates"]:
        k = dev.locusrate_counters()
        out["mui"] = k["mui"][1]
        if c["mubar"]:
            out["mubar"] = k["mubar"][1]
    if c["subst"]:                              # (summary()'s count pools the parameter steps with the tree moves: the values tell)
        out["subst"] = [tuple(np.asarray(x).tolist() for x in dev.get_subst_model(i)) for i in range(n)]
    return out


# case, set, options on top of the set's, moves, tail, kind()
TAILS = [
    ("G1", "b12", {}, "program", "whole", "generic"),
    ("G1", "b12", {}, "uniform", "whole", "generic"),
    ("G2", "b12", dict(host_decisions=True), "program", "whole", "generic"),
    ("G3", "b12", {}, "program", "mui-pending", "generic"),
    ("G4", "b12", {}, "uniform", "hrdt", "generic"),
    ("G5", "b12", {}, "uniform", "subst", "generic"),
    ("G6", "d8", {}, "uniform", "mui-mubar", "generic"),
    ("G7", "gtr8", {}, "program", "invgamma", "generic"),
    ("G7", "gtr8", {}, "uniform", "invgamma", "generic"),
    ("G7", "gtr8", dict(host_decisions=True), "program", "invgamma", "generic"),
    ("G7", "gtr8", dict(host_decisions=True), "uniform", "invgamma", "generic"),
    ("G8", "handover-65", dict(chain=False), "program", "none", "generic"),
    ("G8", "handover-65", dict(chain=True), "program", "none", "generic"),
    ("B1", "set17", {}, "program", "whole", "big"),
    ("B1", "set17", {}, "uniform", "whole", "big"),
    ("B2", "set17", {}, "program", "subst", "big"),
    ("B3", "b12-big", {}, "program", "whole", "big"),
    ("B4", "big-17-30", {}, "program", "invgamma", "big"),
    ("B4", "big-17-30", {}, "uniform", "invgamma", "big"),
    ("S1", "jc8-sweep", {}, "uniform", "invgamma", "sweep"),
]


def _tail_id(v):
    if isinstance(v, dict):
        return "+".join(f"{k}={int(x)}" for k, x in v.items()) or "default"
    return None


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("case,name,options,moves,tail,kind", TAILS, ids=_tail_id)
def test_rows_under_the_tails_equal_stop_and_look_and_the_unstopped_chain(case, name, options, moves, tail, kind, every):
    """30 iterations, A as iterate(25) + iterate(5).  Every row: taus and thetas == B's, lnL == the replay of the documented order
    over B's per-locus lnl and within the any-order bound of B's summary().  At the end A, B and C hold the same state (values and
    counters of every feature that is on), and A passes the CPU recompute of that feature set.  Not vacuous: on some row's
    iteration every move of the tail accepted something since B's previous stop, and each component the case names has moved"""
    base, opts = _set(name)
    c = dict(base, subst=False, rates=False, mubar=False, hered=False, gibbs=False)
    c.update(TAIL[tail])
    data, n = c["data"], len(c["data"])
    eng = bpp_amd.Engine(0)
    (A, B, C), loci = three(eng, c, moves, tail, name, dict(opts, **options))
    assert A.kind() == B.kind() == C.kind() == kind
    npop = len(c["stree"][0])
    assert A.trace_width() == 2 + 2*npop
    start = tail_reading(B, c)
    rates0, hered0 = (B.get_locus_rates() if c["rates"] else None), (B.get_heredity() if c["hered"] else None)
    A.set_trace(every, 4096)
    A.iterate(FIRST)
    A.iterate(TOTAL - FIRST)
    rows = A.trace()
    C.iterate(TOTAL)
    want_it = list(range(every, TOTAL + 1, every))
    assert list(rows["iteration"]) == want_it
    assert rows["taus"].shape == rows["thetas"].shape == (len(want_it), npop) and rows["lnl"].shape == (len(want_it),)
    done, prev, hit = 0, start, {k: [] for k in start}
    for r, it in enumerate(want_it):
        B.iterate(it - done)
        done = it
        assert list(rows["taus"][r]) == B.taus() and list(rows["thetas"][r]) == B.thetas(), it
        lnl = np.array([B.tree(i)["lnl"] for i in range(n)])
        replay = replay_parts([lnl])
        total = B.summary()["total_lnl"]
        assert rows["lnl"][r] == replay, (it, rows["lnl"][r], replay)
        assert abs(rows["lnl"][r] - total) <= any_order_bound(lnl), it
        now = tail_reading(B, c)
        for k in now:
            if now[k] != prev[k]:
                hit[k].append(it)
        prev = now
    if done < TOTAL:
        B.iterate(TOTAL - done)
    print(f"[trace-tails] {case} {name} {moves} {options} every {every}: rows on which each tail move had accepted since the stop before: {hit}; "
          f"launches A {A.summary()['launches']} B {B.summary()['launches']} C {C.summary()['launches']}")
    assert all(hit.values()), hit                                  # (no tail: nothing to show)
    assert rows["taus"][-1].tolist() != list(c["stree"][1]) and len(set(rows["lnl"])) > 1          # the chain moved
    assert len(A.trace()["lnl"]) == 0
    sa = state(A, c)
    same_state(sa, state(B, c))
    same_state(sa, state(C, c))
    if c["subst"]:
        f, q, a = moved_components(A, data)
        assert f and q and a, (f, q, a)
    if c["rates"]:
        mui, mubar = A.get_locus_rates()
        assert (mui != rates0[0]).any() and (mubar != rates0[1]) == c["mubar"], (mui, mubar)
        k = A.locusrate_counters()
        assert k["mui"][0] == TOTAL*n and k["mubar"][0] == (TOTAL if c["mubar"] else 0)
    if c["hered"]:
        assert (A.get_heredity() != hered0).any() and A.heredity_counters()[0] == TOTAL*n
    if c["gibbs"]:
        gp, ga = A.gibbs_counters()
        assert (gp > 0 and ga == gp) if moves == "program" else (gp, ga) == (0, 0)       # tests/test_gpu_invgamma.py: every such draw is accepted
    seen = recompute(A, c, loci, tail)
    print(f"[trace-tails] {case} recompute: {seen}")
    for d in (A, B, C):
        d.close()
    eng.close()


# ------------------------------------------------------------------ B. more loci than threads
# (loci, moves, implementation, kind(), the samplers' seed).  The data sets' seeds are 91 (1 025 loci) and 92 (2 500).
# The samplers' seeds are those on which the thread count shows in a row (the test's docstring).  At 2 500 loci the module's
# seed 31 does: row 4 (uniform), row 8 (program).  At 1 025 loci it does not, nor does nearly any other: with 1 024 threads
# thread 0 holds (x0 + x1024) and adds x512 in the tree, with 512 it holds (x0 + x512) + x1024 and every other thread what the
# tree's first level gives, so two orders differ in ONE association of three values of ~1e2, whose last bit must then survive
# nine levels of sums up to ~1e5 (0.07 % of rows on random values of this size).  The seeds were counted up from 101 until
# a row differed: 318 under uniform windows (row 4; the persistent kernel, the generic and the one-launch-per-step sampler
# walk the same chain), 226 with the program's moves (row 8)
MANY_DATA_SEED = {1025: 91, 2500: 92}
MANY = [(1025, "uniform", None, "persistent", 318), (1025, "program", None, "persistent", 226), (2500, "uniform", None, "persistent", SEED),
        (2500, "program", None, "persistent", SEED), (1025, "uniform", "generic", "generic", 318), (1025, "uniform", "sweep", "sweep", 318)]
_MANY = {}


def many(n):
    """n JC69 loci of 4 tips and 40 sites (built once, never changed) -> the dict shapes.configure takes"""
    if n not in _MANY:
        data = synth.make_dataset(n, 40, 4, "jc69", 1, seed=MANY_DATA_SEED[n])
        st4 = synth.species_tree_arrays(4)
        _MANY[n] = shapes._case(f"many-{n}", data, [list(range(4))]*n, st4, None)
    return _MANY[n]


def index_order_sum(values):
    acc = 0.0
    for x in values:
        acc = acc + float(x)
    return acc


def run_many(n, moves, implementation, kind, seed):
    """-> the rows' iterations on which a replay with 512 threads differs from the row"""
    c = many(n)
    assert len(c["data"]) == n > 1024 and max(len(d["weights"]) for d in c["data"]) <= 64
    eng = bpp_amd.Engine(0)
    devs = []
    for _ in range(3):
        devs.append(bpp_amd.Sampler(eng, tape.make_engine_loci(eng, c["data"]), c["data"], seed=seed, implementation=implementation))
        shapes.configure(devs[-1], c, moves)
    for d in devs:
        d.initialize()
    A, B, C = devs
    assert A.kind() == B.kind() == C.kind() == kind
    A.set_trace(4, 4096)
    A.iterate(7)
    A.iterate(5)
    rows = A.trace()
    C.iterate(12)
    assert list(rows["iteration"]) == [4, 8, 12]
    visible, plain = [], []
    for r, it in enumerate([4, 8, 12]):
        B.iterate(4)
        assert list(rows["taus"][r]) == B.taus() and list(rows["thetas"][r]) == B.thetas(), it
        lnl = np.array([B.tree(i)["lnl"] for i in range(n)])
        assert rows["lnl"][r] == replay_sum(lnl), (it, rows["lnl"][r], replay_sum(lnl))
        assert abs(rows["lnl"][r] - B.summary()["total_lnl"]) <= any_order_bound(lnl), it
        if rows["lnl"][r] != replay_sum(lnl, threads=512):
            visible.append(it)
        if rows["lnl"][r] != index_order_sum(lnl):
            plain.append(it)
    print(f"[trace-tails] {n} loci {moves} {kind} seed {seed}: rows that differ from a replay with 512 threads: {visible}, from the sum "
          f"in index order: {plain}; launches A {A.summary()['launches']} C {C.summary()['launches']}")
    assert rows["taus"][-1].tolist() != list(c["stree"][1]) and len(set(rows["lnl"])) == 3
    sa = state(A, c)
    same_state(sa, state(B, c))
    same_state(sa, state(C, c))
    for d in devs:
        d.close()
    eng.close()
    return visible, plain


@pytest.mark.parametrize("n,moves,implementation,kind,seed", MANY, ids=[f"{n}-{m}-{k}" for n, m, _, k, _s in MANY])
def test_rows_of_more_loci_than_threads(n, moves, implementation, kind, seed):
    """trace_row_kernel's `for (i = threadIdx.x; i < n; i += 1024)` beyond its first trip: at 1 025 loci thread 0 adds two
    values, at 2 500 threads 0 .. 451 add three and the rest two.  12 iterations (A: 7 + 5), a row every 4.
    The == against the replay sees the order of the additions only where another order gives another double, so some row must
    differ from the replay with 512 threads (and from the sum in index order)."""
    visible, plain = run_many(n, moves, implementation, kind, seed)
    assert plain, "no row differs from the sum in index order"
    assert visible, "no row differs from a replay with 512 threads: the == does not see the thread count on this chain — another seed"


# ------------------------------------------------------------------ C. hand-over, partial reads, burn-in, re-arming
OFF_PERSISTENT = [("generic-16-gtr-g4", "program"), ("big-17-30", "program"), ("composite-64-65", "uniform")]
off_persistent = pytest.mark.parametrize("name,moves", OFF_PERSISTENT, ids=[n for n, _ in OFF_PERSISTENT])


def row_is(row, dev, c):
    """a raw row [iteration, lnL, taus, thetas] against a stopped sampler: taus, thetas ==, lnL == the parts' replay"""
    npop = len(c["stree"][0])
    assert list(row[2:2 + npop]) == dev.taus() and list(row[2 + npop:]) == dev.thetas(), row[0]
    lnl = np.array([dev.tree(i)["lnl"] for i in range(len(c["data"]))])
    assert row[1] == replay_parts([lnl[p] for p in parts_of(c)]), row[0]


@off_persistent
def test_capacity_and_partial_reads_off_the_persistent_kernel(name, moves):
    """every = 1, 40 iterations: a device buffer of 4 rows (handed to the host ten times) read as 10 + the rest gives the bits
    of a buffer of 64 read at once, iterations 1 .. 40 each once and in order.  The composite also in bites of 7, 1 and the
    rest with iterations in between — its parts' stores take new rows behind a non-zero head — and against an untraced twin
    stopped at 7, 8 and 40"""
    c = shapes.case(name)
    comp = c["kind"] == "composite"
    eng = bpp_amd.Engine(0)
    devs = twins(eng, c, moves, count=4 if comp else 2)
    X, Y = devs[:2]
    assert all(d.kind() == c["kind"] for d in devs)
    w = X.trace_width()
    assert w == 2 + 2*len(c["stree"][0])
    X.set_trace(1, 64); Y.set_trace(1, 4)
    X.iterate(40); Y.iterate(40)
    big = X.trace_read()
    assert big.shape == (40, w) and list(big[:, 0]) == list(range(1, 41))
    r1 = Y.trace_read(10)
    r2 = Y.trace_read()
    assert r1.shape == (10, w) and r2.shape == (30, w)
    assert np.array_equal(np.concatenate([r1, r2]), big)
    assert len(X.trace_read()) == 0 and len(Y.trace_read()) == 0
    sx = state(X, c)
    same_state(sx, state(Y, c))
    assert len(set(big[:, 1])) > 1 and list(big[-1, 2:]) != list(big[0, 2:])                  # the chain moved
    if comp:
        Z, U = devs[2:]
        Z.set_trace(1, 4)
        Z.iterate(25)
        b1 = Z.trace_read(7)
        Z.iterate(15)
        b2 = Z.trace_read(1)
        b3 = Z.trace_read()
        assert (len(b1), len(b2), len(b3)) == (7, 1, 32)
        assert np.array_equal(np.concatenate([b1, b2, b3]), big)
        same_state(sx, state(Z, c))
        for stop, step in ((7, 7), (8, 1), (40, 32)):
            U.iterate(step)
            row_is(big[stop - 1], U, c)
        same_state(sx, state(U, c))
    for d in devs:
        d.close()
    eng.close()


@off_persistent
def test_burnin_writes_no_row_off_the_persistent_kernel(name, moves):
    """set_trace(1, 16): burnin(40) writes no row; nor does burnin(200), where the step-length rule runs (the generic and the
    big-tree sampler: the rule does not run on a composite) and returns an untraced twin's step lengths; iterate(3) afterwards
    gives rows 1, 2, 3, which are the twin's taus and thetas, and the same final state"""
    c = shapes.case(name)
    eng = bpp_amd.Engine(0)
    dev, ref = twins(eng, c, moves)
    assert dev.kind() == ref.kind() == c["kind"]
    dev.set_trace(1, 16)
    ft0 = dev.burnin(40)
    assert ft0 == ref.burnin(40)
    assert len(dev.trace_read()) == 0
    if c["kind"] != "composite":
        ft = dev.burnin(200)
        assert ft == ref.burnin(200) and ft != ft0, (ft, ft0)              # (the rule ran: the lengths changed)
        assert len(dev.trace_read()) == 0
    dev.iterate(3)
    rows = dev.trace_read()
    assert list(rows[:, 0]) == [1, 2, 3]
    for r in range(3):
        ref.iterate(1)
        row_is(rows[r], ref, c)
    same_state(state(dev, c), state(ref, c))
    dev.close(); ref.close(); eng.close()


@off_persistent
def test_a_second_set_trace_starts_over_off_the_persistent_kernel(name, moves):
    """set_trace(2, 16), iterate(5), set_trace(3, 16) without reading, iterate(7): rows [3, 6] only — the count starts over and
    the first trace's unread rows (2, 4) are gone —, which are what an untraced twin shows after 8 and 11 iterations; the
    state is that of an untraced iterate(12); then set_trace(0, 0): iterate(2) gives no row"""
    c = shapes.case(name)
    eng = bpp_amd.Engine(0)
    dev, ref, stop = twins(eng, c, moves, count=3)
    assert dev.kind() == ref.kind() == stop.kind() == c["kind"]
    dev.set_trace(2, 16)
    dev.iterate(5)
    dev.set_trace(3, 16)
    dev.iterate(7)
    rows = dev.trace_read()
    assert list(rows[:, 0]) == [3, 6]
    ref.iterate(12)
    stop.iterate(8)
    row_is(rows[0], stop, c)
    stop.iterate(3)
    row_is(rows[1], stop, c)
    stop.iterate(1)
    sd = state(dev, c)
    same_state(sd, state(ref, c))
    same_state(sd, state(stop, c))
    dev.set_trace(0, 0)
    dev.iterate(2); ref.iterate(2)
    assert len(dev.trace_read()) == 0
    same_state(state(dev, c), state(ref, c))
    for d in (dev, ref, stop):
        d.close()
    eng.close()
