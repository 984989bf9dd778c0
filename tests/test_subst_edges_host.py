"""What the substitution-parameter edge tests (tests/test_gpu_subst_edges.py) rest on, settled without a GPU: the oracle at the
edge eigensystems, and the C host driver on the REAL reference's likelihood from the starts at the moves' reflection bounds —
the seeds of the device runs are chosen here."""
import numpy as np
import pytest

import bpp_amd
import gammadev
import hostdrv
import oraclelib as O
import substedges as E

needs_ref = pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref not built")


def test_the_oracle_at_the_edge_eigensystems():
    """finite eigensystems, P-matrix rows that sum to 1 within 3e-14, benign conditioning: max (|W||V|) <= 2.4 — the factor in
    the GPU test's P-matrix bar"""
    rates = bpp_amd.compute_gamma_cats(0.7, 0.7, 4)
    for name, f, q in E.EIGEN_CASES:
        assert abs(sum(f) - 1) < 1e-15, name
        ev, iev, evals = O.orc_eigen(np.array(f, dtype=float), np.array(q, dtype=float))
        assert np.isfinite(ev).all() and np.isfinite(iev).all() and np.isfinite(evals).all(), name
        assert (np.abs(iev) @ np.abs(ev)).max() <= 2.4, name
        assert np.sort(evals)[-1] < 1e-14 and np.sort(evals)[-2] < -1e-5, (name, evals)        # one zero eigenvalue, the rest negative
        for t in E.BRANCH_LENGTHS:
            for lib in (False, True):
                P = O.orc_pmatrix_eigen(rates, t, evals, ev, iev, library_form=lib)
                assert np.abs(P.sum(axis=-1) - 1).max() < 3e-14, (name, t)
                assert P.min() > -1e-15, (name, t, P.min())
    # the shapes with repeated eigenvalues have them
    for case, mult in ((0, 3), (1, 2), (2, 3)):
        _, f, q = E.EIGEN_CASES[case]
        evals = np.sort(O.orc_eigen(np.array(f, dtype=float), np.array(q, dtype=float))[2])
        assert np.allclose(evals[:mult], evals[0], rtol=1e-14), (case, evals)


def _run(data, seed, windows, taxa, R, iters, each):
    drv = hostdrv.reference_driver(data, seed=seed)
    E.configure(drv, taxa, windows, R, data, host=True)
    drv.initialize()
    for it in range(iters):
        drv.iterate()
        each(drv, it)
    drv.close()


@needs_ref
def test_lower_bound_start_comes_back_from_the_floor():
    """the seed of tests/test_gpu_subst_edges.py::test_moves_at_the_lower_reflection_bound: on the C driver some locus ends an
    iteration with its moved frequency or exchangeability inside [1e-5, 1.2e-5), and none goes below 1e-5"""
    s = E.BOUND_SHAPE
    data, which = E.lower_bound_data()
    assert all(d["freqs"][w[0]] == E.NEAR_FLOOR and d["exch"][w[1]] == E.NEAR_FLOOR and abs(d["freqs"].sum() - 1) < 1e-15
               and w[0] != E.FREQ_REF and w[1] != E.Q_REF for d, w in zip(data, which))
    hits = []

    def each(drv, it):
        for i in range(s["nloci"]):
            m = drv.get_subst_model(i)
            assert min(m[0][:3]) >= E.FLOOR * (1 - 2.0 ** -52) and min(m[1][j] for j in E.Q_MOVED) >= E.FLOOR * (1 - 2.0 ** -52), (it, i, m)
            hits.extend((it, i, what) for what in E.at_floor(m, which[i]))
    _run(data, E.LOWER_SEED, s["windows"], s["taxa"], s["R"], s["iters"], each)
    assert len(hits) >= 4 and {"freq", "exch"} == {h[2] for h in hits}, hits


@needs_ref
@pytest.mark.parametrize("K", gammadev.CATS)
def test_gamma_grid_run_moves_every_alpha(K):
    """the seed of tests/test_gpu_subst_edges.py::test_device_gamma_rates_across_every_branch, set up as its sampler is (BPP's
    kernel, the program's moves): on the C driver every grid alpha's locus has left its grid value by the third iteration — an
    alpha proposal of that locus was accepted, so the device test's checkpoints see rates made for it — and some iteration of
    some locus ends with the alpha it began with"""
    grid = [float(a) for a in gammadev.GRID]
    data = E.gamma_grid_data(grid, K)
    parent, tau0, thetas = bpp_amd.synth.species_tree_arrays(4)
    drv = hostdrv.reference_driver(data, seed=E.GAMMA_SEED)
    drv.set_proposal_kernel(1)
    drv.set_program_moves(True, 0.3)
    drv.set_species_tree(parent, tau0, thetas)
    drv.set_tau_prior(3.0, 3.0 / tau0[-1])
    drv.set_theta_prior(2.0, 1000.0, 0.0004)
    drv.set_finetune(*E.GAMMA_FINETUNE)
    drv.set_subst_moves(*E.GAMMA_WINDOWS, 1.0, 1.0)
    for i, d in enumerate(data):
        drv.set_subst_model(i, list(d["freqs"]), list(d["exch"]), d["alpha"], K)
    drv.initialize()
    alpha, kept = list(grid), 0
    for it in range(1, E.GAMMA_ITERS + 1):
        drv.iterate()
        now = [drv.get_subst_model(i)[2] for i in range(len(grid))]
        kept += sum(a == b for a, b in zip(now, alpha))
        alpha = now
        if it == 3:
            assert all(a != g for a, g in zip(alpha, grid)), [g for a, g in zip(alpha, grid) if a == g]
    assert all(a != g for a, g in zip(alpha, grid)) and kept > 0, kept
    drv.close()


@needs_ref
def test_upper_bound_start_on_the_c_driver():
    """f = (.3, .3, .4 - 1e-9, 1e-9) with windows of 3.0 on the C driver (the arithmetic of locus.c:2819-2833): no frequency is
    non-positive at the end of an iteration, the frequencies sum to 1 within 4 ulp, every likelihood is finite — the start of
    the device test needs no moving"""
    s = E.BOUND_SHAPE
    data = E.upper_bound_data()
    # the start sits at the bound: each moved frequency is within 4e-9 of log(sum) (sum = itself + the reference's 1e-9) against a
    # half-window of 1.5, so every upward draw but one in 4e8 overshoots log(sum) and is reflected; each locus draws three such
    # windows in its first iteration alone.  (The state an iteration leaves cannot tell a reflected upward proposal from a
    # downward one of the same length: from this start the two land within 7e-9 relative of each other.)
    for d in data:
        f = d["freqs"]
        assert all(0 < np.log(f[j] + f[E.FREQ_REF]) - np.log(f[j]) < 4e-9 for j in range(3)), f
    assert s["windows"][0] / 2 == 1.5

    def each(drv, it):
        for i in range(s["nloci"]):
            f, q, a = drv.get_subst_model(i)
            assert min(f) > 0 and min(q) > 0 and np.isfinite(f).all() and np.isfinite(q).all(), (it, i, f, q)
            assert abs((f[0] + f[1] + f[2] + f[3]) - 1.0) <= 4 * 2.0 ** -52, (it, i, f)
            assert np.isfinite(drv.tree(i)["lnl"]), (it, i)
    _run(data, E.UPPER_SEED, s["windows"], s["taxa"], s["R"], s["iters"], each)


@needs_ref
def test_wide_windows_from_the_edge_eigensystems_reject_and_accept():
    """the seed of the GPU test's wide-windows sampler run: after one iteration some parameter vector is as at the start (every
    move of it rejected and put back) and most have moved"""
    data = E.eigen_case_data()
    seen = {}

    def each(drv, it):
        moved = kept = 0
        for i, (_, f, q) in enumerate(E.EIGEN_CASES):
            ff, qq, _ = drv.get_subst_model(i)
            for x, y in ((ff, f), (qq, q)):
                moved += int(list(x) != list(y)); kept += int(list(x) == list(y))
            assert np.isfinite(drv.tree(i)["lnl"]) and min(ff) > 0 and min(qq) > 0, i
        seen["moved"], seen["kept"] = moved, kept
    _run(data, E.EIGEN_SEED, (3.0, 3.0, 0.8), 4, 4, 1, each)
    assert seen["kept"] >= 2 and seen["moved"] >= 10, seen
