"""The substitution-parameter path of the generic sampler (BASELINE config 3's kind: GTR + Gamma) at its branch points and bounds.

a. The device's discrete-gamma rates (csrc/gamma_dev.hpp, run by gsampler.hpp's write_par for every alpha proposal and every
   rejected one), read back with Locus.get_category_rates, against bpa_compute_gamma_cats over a grid of shapes that takes every
   start-value branch of chi2_quantile, the Wilson-Hilferty correction and both forms of incomplete_gamma.  The bar at a grid
   point is 8 x the spread that +-1 ulp on every exp / log / pow gives the HOST build of the same text
   (tests/golden/gamma_dev_sensitivity.json, tests/golden/make_golden_gamma_dev.py; CPU twin: tests/test_gamma_dev_host.py).
b. K6 on the device (kernels.hpp: update_eigen_regs<4> / eigen_sym_static) at eigensystems with repeated eigenvalues, frequencies
   at and below the moves' floor, exchangeabilities at the floor and far above it — through bpa_update_eigen, the per-locus
   setters, bpa_plan_set_params, a sampler's start-up and the sampler's own moves (fused into gstep_kernel<6|7>, and
   eigen_kernel<4> when a gene-tree step settles the last exchangeability move) — == the oracle's, then P-matrices.
c. The frequency / exchangeability moves at the two ends of reflect(.., log 1e-5, log sum).

What one MI355X showed at each of these is in NOTES.md, section 14.
"""
import numpy as np
import pytest

import bpp_amd
from bpp_amd import synth
from bpp_amd.api import PARAM_FREQS, PARAM_SUBST
import gammadev
import hostdrv
import oraclelib as O
import substedges as E
import tape
from invariants import check_state, ulps, PMAT_ULPS, PMAT_ATOL
from test_gpu_gsampler import walk
from test_gpu_params import full_plan
from test_gpu_state_invariants import make

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ a. category rates
# the loci whose oracle in check_state takes the DEVICE's rates (held to their own bar first): the grid shapes from here on, where
# the last places of libm move a rate by 4e-13 .. 1.3e-11 (the fixture) — which these trees' off-diagonal P-matrix entries of
# 2e-3 .. 7e-3 show as 1e-15 .. 1e-13, beyond the P-matrix bar of 8 ulp / 5e-16 (seen at one such locus: NOTES.md, section 14);
# every other locus's oracle takes the host routine's rates for the device's alpha
DEVICE_RATES_FROM = 100.0


def gamma_grid_sampler(K):
    """31 four-tip GTR loci of 40 sites, one per grid alpha, on a generic sampler with the program's moves; the frequency and
    exchangeability windows of 1e-6 keep those moves on without moving anything, the alpha window of 0.05 moves alpha by ~1e-2
    relative -> (engine, sampler, engine loci, data, species tree, grid)"""
    grid = [float(a) for a in gammadev.GRID]
    eng = bpp_amd.Engine(0)
    data = E.gamma_grid_data(grid, K)
    stree = synth.species_tree_arrays(4)
    dev, loci = make(eng, data, stree, E.GAMMA_SEED, "program", finetune=E.GAMMA_FINETUNE)
    dev.set_subst_moves(*E.GAMMA_WINDOWS, 1.0, 1.0)
    for i, d in enumerate(data):
        dev.set_subst_model(i, d["freqs"], d["exch"], d["alpha"])
    dev.initialize()
    return eng, dev, loci, data, stree, grid


@pytest.mark.parametrize("K", gammadev.CATS)
def test_device_gamma_rates_across_every_branch(K):
    """a block left holding a rejected proposal's rates is off by eight orders of magnitude more than the bar (the seed is
    chosen on the CPU: tests/test_subst_edges_host.py has every locus's alpha off its grid value by the third iteration)"""
    bars = gammadev.load_bars()
    eng, dev, loci, data, stree, grid = gamma_grid_sampler(K)
    n, iters = len(grid), E.GAMMA_ITERS
    assert dev.kind() == "generic"
    for i, d in enumerate(data):                     # before any move the block holds what the host uploaded
        assert (loci[i].get_category_rates() == d["rates"]).all(), i
    p0 = dev.summary()["proposals"]
    alpha = list(grid)
    kept, changed = [0] * n, [0] * n                 # per locus: iterations that ended with the alpha they began with / another
    remade = [False] * n                             # per locus: a checkpoint found the rates of an alpha that is not the grid's
    worst, worst_share, worst_mean = 0.0, 0.0, 0.0
    for it in range(1, iters + 1):
        dev.iterate(1)
        now = [dev.get_subst_model(i)[2] for i in range(n)]
        for i in range(n):
            kept[i] += now[i] == alpha[i]
            changed[i] += now[i] != alpha[i]
        alpha = now
        if it not in (1, 3, 6):
            continue
        for i in range(n):
            a = alpha[i]
            got = loci[i].get_category_rates()
            want = bpp_amd.compute_gamma_cats(a, a, K)
            bar = gammadev.bar(bars, a, K)
            err = np.abs(got - want) / want
            print(f"[subst-edges] K {K} iteration {it} alpha {a:.6g}: rates off by {err.max():.2e} (bar {bar:.2e}), mean - 1 = {got.mean() - 1:.2e}")
            assert np.isfinite(got).all() and (got > 0).all() and (np.diff(got) > 0).all(), (it, a, got)
            assert (err <= bar).all(), f"alpha {a!r}, {K} categories, iteration {it}: device rates {got} vs host {want}: off by {err.max():.3e}, bar {bar:.3e}"
            assert abs(got.mean() - 1) <= bar, (it, a, got.mean() - 1, bar)
            remade[i] |= a != grid[i]
            worst, worst_share, worst_mean = max(worst, err.max()), max(worst_share, err.max() / bar), max(worst_mean, abs(got.mean() - 1))
    print(f"[subst-edges] K {K}: largest device-vs-host rate difference {worst:.2e}, largest share of its bar {worst_share:.3f}, "
          f"largest |mean - 1| {worst_mean:.2e}; alpha kept {sum(kept)}, changed {sum(changed)} of {n * iters} locus-iterations; "
          f"loci that kept it at least once: {[i for i in range(n) if kept[i]]}")
    # both outcomes occurred: rates re-made for a rejected proposal's old alpha and rates of an accepted one
    assert sum(kept) > 0 and sum(changed) > 0, (kept, changed)
    # every grid alpha's locus had an alpha proposed, locus by locus: its alpha left the grid value (only an accepted proposal
    # does that), and a checkpoint then held the block to the rates of that other alpha, orders of magnitude more
    # closely than the grid value's rates are to them — rates the host never uploaded, so the device made them
    never = [grid[i] for i in range(n) if not (changed[i] and remade[i])]
    assert not never, f"{K} categories: the loci of these grid alphas never showed the rates of a proposed alpha: {never}"
    # the counter, for what a sum can say: more than the gene-tree steps (3 age + 6 prune-regraft a locus-iteration) and the
    # all-loci steps (a theta a population, a tau an inner one, a mix: under 2 a population) can add up to
    grew = dev.summary()["proposals"] - p0
    print(f"[subst-edges] K {K}: {grew} proposals in {iters} iterations of {n} loci")
    assert grew > iters * (9 * n + 2 * len(stree[0])), grew
    # the whole state against a recompute
    late = {i for i in range(n) if grid[i] >= DEVICE_RATES_FROM}
    check_state(dev, data, stree[0], loci=loci, subst=True, rates_of=lambda i: loci[i].get_category_rates() if i in late else None)
    dev.close(); eng.close()


# ------------------------------------------------------------------------------------------------ b. K6 at the edges
_ORACLE = {}
RATES = None


def oracle_eigen(f, q):
    key = (tuple(float(x) for x in f), tuple(float(x) for x in q))
    if key not in _ORACLE:
        e = O.orc_eigen(np.array(key[0]), np.array(key[1]))
        assert all(np.isfinite(x).all() for x in e), key
        _ORACLE[key] = e
    return _ORACLE[key]


def same_eigen(got, f, q, what):
    want = oracle_eigen(f, q)
    for name, g, w in zip(("eigenvectors", "inverse eigenvectors", "eigenvalues"), got, want):
        assert (g == w).all(), f"{what}: {name} differ from the oracle's for f = {list(f)}, q = {list(q)}: largest difference {np.abs(g - w).max():.3e}\n{g}\n{w}"
    return want


def check_pmatrices(engine, loc, eig, what):
    """entrywise <= 8 ulp or 5e-16 max(1, (|W||V|)ij): the project's bar (tests/test_gpu_parity.py), scaled by the factor by which a
    1-ulp expm1 difference in every eigen-term reaches that entry; equal to it wherever |W||V| <= 1"""
    global RATES
    if RATES is None:
        RATES = bpp_amd.compute_gamma_cats(0.7, 0.7, 4)
    ev, iev, evals = eig
    scale = np.maximum(1.0, np.abs(iev) @ np.abs(ev))
    bl = np.array(E.BRANCH_LENGTHS)
    lib_form = engine.core_update_pmatrix(4, RATES, bl, evals, ev, iev)
    loc.set_category_rates(RATES)
    loc.update_matrices(np.arange(len(bl)), bl)
    worst_u = worst_a = 0.0
    for k, t in enumerate(bl):
        for form, got in (("library", lib_form[k]), ("locus", loc.get_pmatrix(k))):
            want = O.orc_pmatrix_eigen(RATES, float(t), evals, ev, iev, library_form=(form == "library"))
            u, a = ulps(got, want), np.abs(got - want)
            ok = (u <= PMAT_ULPS) | (a < PMAT_ATOL * scale)
            assert ok.all(), f"{what}, t = {t}, {form} form: {u[~ok].max():.1f} ulp / {a[~ok].max():.3e} absolute (|W||V| up to {scale.max():.2f})"
            assert np.allclose(got.sum(axis=-1), 1.0, atol=1e-12)
            worst_u = max(worst_u, u[u <= PMAT_ULPS].max(initial=0.0))
            worst_a = max(worst_a, (a / scale)[u > PMAT_ULPS].max(initial=0.0))
    assert (lib_form[0] == np.eye(4)).all()
    print(f"[subst-edges] {what}: P-matrices within {worst_u:.0f} ulp, beyond that {worst_a:.2e} / max(1, |W||V|) absolute (|W||V| up to {scale.max():.2f})")


@pytest.mark.parametrize("case", range(len(E.EIGEN_CASES)), ids=[c[0].replace(" ", "-") for c in E.EIGEN_CASES])
def test_edge_eigensystem_by_engine_setters_and_plan(engine, case):
    name, f, q = E.EIGEN_CASES[case]
    f, q = np.array(f, dtype=float), np.array(q, dtype=float)
    want = same_eigen(engine.update_eigen(f, q, 4), f, q, f"{name}: bpa_update_eigen")
    # loci made with the synthetic model's parameters, then moved to the case's: frequencies first (an eigensystem of the case's
    # frequencies with the old exchangeabilities in between), then exchangeabilities
    d = synth.make_dataset(2, 40, 4, "gtr", 4, seed=57)
    a, b = tape.make_engine_loci(engine, d)
    a.set_frequencies(0, f)
    same_eigen(a.get_eigen(0), f, d[0]["exch"], f"{name}: bpa_set_frequencies")
    a.set_subst_params(0, q)
    same_eigen(a.get_eigen(0), f, q, f"{name}: bpa_set_subst_params")
    plan = full_plan(engine, [b], d[1:])
    plan.set_params(PARAM_SUBST, q[None, :])
    same_eigen(b.get_eigen(0), d[1]["freqs"], q, f"{name}: bpa_plan_set_params(PARAM_SUBST)")
    plan.set_params(PARAM_FREQS, f[None, :])
    same_eigen(b.get_eigen(0), f, q, f"{name}: bpa_plan_set_params(PARAM_FREQS)")
    check_pmatrices(engine, a, want, name)
    plan.launch()
    assert np.isfinite(plan.lnl()).all()
    plan.close()


# (frequency and exchangeability windows, alpha window, iterations)
SAMPLER_RUNS = {"tiny-windows": (1e-9, 0.05, 1),        # proposals an ulp-scale step away from the edge values: K6 fused into the move
                "wide-windows": (3.0, 0.8, 1),          # ... about half of them rejected: the restore path's K6, starting from the edges
                "no-alpha-move": (1e-9, 0.0, 2)}        # the last exchangeability move settled by a gene-tree step: eigen_kernel<4>


@pytest.mark.parametrize("run", list(SAMPLER_RUNS))
def test_edge_eigensystems_in_a_sampler(run):
    w, wa, iters = SAMPLER_RUNS[run]
    eng = bpp_amd.Engine(0)
    data = E.eigen_case_data()
    n = len(data)
    loci = tape.make_engine_loci(eng, data)
    dev = bpp_amd.Sampler(eng, loci, data, seed=E.EIGEN_SEED)
    E.configure(dev, 4, (w, w, wa), data=data)
    dev.initialize()
    assert dev.kind() == "generic"
    start = [dev.get_subst_model(i) for i in range(n)]
    for i, (name, f, q) in enumerate(E.EIGEN_CASES):
        assert (start[i][0] == np.array(f)).all() and (start[i][1] == np.array(q)).all()
        same_eigen(loci[i].get_eigen(0), f, q, f"{name}: sampler after initialize")
        assert np.isfinite(dev.tree(i)["lnl"]), name
    dev.iterate(iters)
    moved = kept = 0
    for i, (name, _, _) in enumerate(E.EIGEN_CASES):
        f, q, _ = dev.get_subst_model(i)
        assert np.isfinite(f).all() and np.isfinite(q).all() and (f > 0).all() and (q > 0).all(), (name, f, q)
        same_eigen(loci[i].get_eigen(0), f, q, f"{name}: sampler after {iters} iteration(s), {run}")
        assert np.isfinite(dev.tree(i)["lnl"]), name
        for x, y in ((f, start[i][0]), (q, start[i][1])):
            moved += int((x != y).any()); kept += int((x == y).all())
    print(f"[subst-edges] sampler, {run}: {moved} parameter vectors moved, {kept} as at the start, of {2 * n}")
    assert moved > 0
    if run == "wide-windows":                # some vector is as at the start: each of its moves was rejected and put back
        assert kept > 0
    dev.close(); eng.close()


# ------------------------------------------------------------------------------------------------ c. the moves' bounds
def test_moves_at_the_lower_reflection_bound():
    """one frequency and one exchangeability of every locus start at 1.2e-5, the windows of 3.0 overshoot log 1e-5: the device
    sampler walks the host driver's trajectory (nothing cancels at this end), and some locus ends an iteration with such a
    component inside [1e-5, 1.2e-5) — a proposal that came back from the floor, accepted (the seed is chosen on the CPU:
    tests/test_subst_edges_host.py shows the same on the reference's own likelihood)"""
    s = E.BOUND_SHAPE
    eng = bpp_amd.Engine(0)
    data, which = E.lower_bound_data()
    loci_a, loci_b = tape.make_engine_loci(eng, data), tape.make_engine_loci(eng, data)
    host = hostdrv.hip_driver(eng, loci_a, data, seed=E.LOWER_SEED)
    dev = bpp_amd.Sampler(eng, loci_b, data, seed=E.LOWER_SEED)
    E.configure(host, s["taxa"], s["windows"], s["R"], data, host=True)
    stree = E.configure(dev, s["taxa"], s["windows"], data=data)
    hits = []

    def each(it):
        for i in range(s["nloci"]):
            m = dev.get_subst_model(i)
            assert min(m[0][:3]) >= E.FLOOR * (1 - 2.0 ** -52) and min(m[1][j] for j in E.Q_MOVED) >= E.FLOOR * (1 - 2.0 ** -52), (it, i, m)
            hits.extend((it, i, what) for what in E.at_floor(m, which[i]))

    walk(host, dev, s["iters"], s["nloci"], each=each)
    for i in range(s["nloci"]):
        fh, qh, ah = host.get_subst_model(i)
        fd, qd, ad = dev.get_subst_model(i)
        assert np.allclose(fd, fh, rtol=1e-11, atol=0) and np.allclose(qd, qh, rtol=1e-11, atol=0) and abs(ad - ah) <= 1e-11 * ah, i
    print(f"[subst-edges] lower bound: {len(hits)} (iteration, locus, component) inside [1e-5, 1.2e-5): {hits[:8]}")
    assert hits
    check_state(dev, data, stree[0], loci=loci_b, subst=True)
    dev.close(); host.close(); eng.close()


def test_moves_at_the_upper_reflection_bound():
    """every locus starts at f = (.3, .3, .4 - 1e-9, 1e-9): nearly every upward proposal of a frequency reflects at log(sum), and
    v[ref] = sum - exp(l_new) cancels — device and glibc exp legitimately differ by ~1e-7 relative in v[ref], so no host
    trajectory is compared; the state itself must stay sane after every iteration, and level with a recompute from the device's
    own current parameters at the end"""
    s = E.BOUND_SHAPE
    eng = bpp_amd.Engine(0)
    data = E.upper_bound_data()
    loci = tape.make_engine_loci(eng, data)
    dev = bpp_amd.Sampler(eng, loci, data, seed=E.UPPER_SEED)
    stree = E.configure(dev, s["taxa"], s["windows"], data=data)
    dev.initialize()
    smallest = 1.0
    for it in range(s["iters"]):
        dev.iterate(1)
        for i in range(s["nloci"]):
            f, q, a = dev.get_subst_model(i)
            assert np.isfinite(f).all() and np.isfinite(q).all() and (f > 0).all() and (q > 0).all() and a > 0, (it, i, f, q, a)
            assert abs(float(f[0] + f[1] + f[2] + f[3]) - 1.0) <= 4 * 2.0 ** -52, (it, i, f, f.sum() - 1)
            assert min(f[:3]) >= E.FLOOR * (1 - 2.0 ** -52) and min(q[j] for j in E.Q_MOVED) >= E.FLOOR * (1 - 2.0 ** -52), (it, i, f, q)
            assert np.isfinite(dev.tree(i)["lnl"]), (it, i)
            smallest = min(smallest, f[E.FREQ_REF])
    moved = sum(dev.get_subst_model(i)[0][E.FREQ_REF] != data[i]["freqs"][E.FREQ_REF] for i in range(s["nloci"]))
    print(f"[subst-edges] upper bound: smallest reference frequency at an iteration's end {smallest:.3e}; {moved} of {s['nloci']} loci left the start")
    assert moved > 0
    check_state(dev, data, stree[0], loci=loci, subst=True)
    dev.close(); eng.close()
