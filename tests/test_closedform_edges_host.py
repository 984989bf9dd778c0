"""What the closed-form edge tests on the device (tests/test_gpu_closedform_edges.py) rest on, settled without a GPU: the oracle's
double form of K80 / F81 / HKY / T92 / TN93 / F84 (pinned bit-exact to the reference, tests/test_oracle_pin.py) against the exact
twin of tests/k7.py over EDGE_CASES x BL, the properties of the exact twin, and the seeds of the bound walks on the C host driver
with the REAL reference's likelihood.  The distances printed here are in NOTES.md, section 29."""
from decimal import Decimal as D

import numpy as np
import pytest

import closedform as CF
import k7
import oraclelib as O
import substedges as E

needs_ref = pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref not built")
ONE = np.ones(1)

# the cases at which the reference's own double form is farther from its exact value than the bar; there the device would be held
# to the oracle only.  None was found: the set stays as the place to name one
FORM_BEYOND_BAR = set()


def oracle_matrix(model, f, q, bl):
    return O.orc_pmatrix_dna(model, np.array(f, dtype=float), k7.padded(q), ONE, float(bl))[0]


@pytest.mark.parametrize("model", CF.CLOSED)
def test_oracle_against_the_exact_twin(model):
    """every entry of the oracle's matrix within 8 ulp or 5e-16 max(1, S) of the form's exact value at the same doubles; the
    largest distance in units of 2^-53 max(1, S) is printed per model (the absolute bar is 4.5 of them)"""
    worst, where, beyond = 0.0, None, {}
    for name, m, f, q in k7.cases_of(model):
        for bl in k7.BL:
            ok, dist = k7.exact_distance(m, f, k7.padded(q), bl, oracle_matrix(m, f, q, bl))
            if name in FORM_BEYOND_BAR:
                beyond[name] = max(beyond.get(name, 0.0), float(dist.max()))
                continue
            if dist.max() > worst:
                worst, where = float(dist.max()), (name, bl)
            assert ok.all(), f"{name}, bl = {bl}: the oracle is {dist[~ok].max():.2f} x 2^-53 max(1, S) from the exact value"
    print(f"[k7 host] {model}: the reference's form is within {worst:.2f} x 2^-53 max(1, S) of its exact value (at {where}); "
          f"beyond the bar by its own form: {beyond}")
    for name, v in beyond.items():
        assert v > 4.5, f"{name} is listed as beyond the bar and is not: {v}"


@pytest.mark.parametrize("model", CF.CLOSED)
def test_properties_of_the_exact_twin(model):
    """rows sum to 1, entries >= 0, pi_i P_ij = pi_j P_ji, P(0) = I, P(1e3) = the stationary vector in every row — on the exact
    twin to 1e-50 (T92 with its rows in the order of the states, k7.T92_ROW: the reference writes them in another); on the oracle
    within the bar"""
    tiny = D("1e-50")
    for name, m, f, q in k7.cases_of(model):
        pi = k7.stationary(m, f)
        if m != "t92":
            assert abs(sum(pi) - 1) < D("1e-15"), name
        for bl in k7.BL:
            P, S = k7.exact_pmatrix(m, f, k7.padded(q), bl)
            Ps = k7.rows_by_state(m, P)
            got = oracle_matrix(m, f, q, bl)
            gs = np.array(k7.rows_by_state(m, [list(r) for r in got]))
            Sf = np.maximum(1.0, np.array(k7.rows_by_state(m, [[float(x) for x in r] for r in S])))
            bar = 8 * 2.0 ** -52 * Sf                   # what level() allows an entry: 8 ulp of a value <= S, or 5e-16 S
            for i in range(4):
                # (F81's rows sum to 1 - expm1(..) (sum f - 1), and the doubles' frequencies sum to 1 within 1e-16 only)
                assert abs(sum(Ps[i]) - 1) <= tiny * 10 + abs(sum(pi) - 1), (name, bl, i)
                assert abs(gs[i].sum() - 1) <= 4 * bar[i].sum(), (name, bl, i, gs[i].sum() - 1)
                for j in range(4):
                    assert Ps[i][j] >= -tiny, (name, bl, i, j, Ps[i][j])
                    assert gs[i, j] >= -bar[i, j], (name, bl, i, j, gs[i, j])
                    assert abs(pi[i] * Ps[i][j] - pi[j] * Ps[j][i]) < tiny, (name, bl, i, j)
                    if name not in FORM_BEYOND_BAR:
                        assert abs(float(pi[i]) * gs[i, j] - float(pi[j]) * gs[j, i]) <= float(pi[i]) * bar[i, j] + float(pi[j]) * bar[j, i] + 1e-300, (name, bl, i, j)
                    if bl == 0.0:
                        assert Ps[i][j] == (1 if i == j else 0) and gs[i, j] == (1.0 if i == j else 0.0), (name, i, j)
            if bl == 1e3 and _mixes(m, f, q):
                # (the limit of the HKY family's rows is f_j (1 - (sum f - 1)/R) or .../Y: f_j where the doubles sum to 1 exactly)
                slack = D("1e-30") + abs(sum(pi) - 1) / min(pi[0] + pi[2], pi[1] + pi[3])
                for i in range(4):
                    for j in range(4):
                        assert abs(Ps[i][j] - pi[j]) <= slack, (name, i, j, Ps[i][j], pi[j])
                        assert abs(gs[i, j] - float(pi[j])) <= 2 * bar[i, j] + float(slack), (name, i, j)


def _mixes(model, f, q):
    """bl = 1e3 has reached the stationary vector: the slowest rate x 1e3 is beyond 70 (e^-70 < 1e-30).  At the floor cases the
    slowest rate itself is of the floor's order, and 1e3 is not long: those are held by the other properties"""
    P, _ = k7.exact_pmatrix(model, f, k7.padded(q), 1e3)
    P2, _ = k7.exact_pmatrix(model, f, k7.padded(q), 2e3)
    return all(abs(P[i][j] - P2[i][j]) < D("1e-31") for i in range(4) for j in range(4))


def test_the_case_table():
    names = [c[0] for c in k7.EDGE_CASES]
    assert len(set(names)) == len(names) and k7.K80_BRANCH in names
    for name, m, f, q in k7.EDGE_CASES:
        assert abs(sum(f) - 1) < 2e-16 and len(q) == CF.TABLE[m][0], name
        assert m != "k80" or f == k7.UNIFORM
    # the stationary check is not vacuous: every model has cases that reach it
    for m in CF.CLOSED:
        assert sum(_mixes(m, f, q) for _, mm, f, q in k7.cases_of(m)) >= 1, m
    # K80's own branch: kappa == 1 takes it, kappa = 1 + 2^-52 does not
    assert abs(1.0 / 1.0 - 1) < 1e-20 and not abs((1.0 + 2.0 ** -52) / 1.0 - 1) < 1e-20
    a, b = oracle_matrix("k80", k7.UNIFORM, (1.0, 1.0), 0.3), oracle_matrix("k80", k7.UNIFORM, (1.0, 1.0 + 2.0 ** -52), 0.3)
    assert len(set(a.ravel())) == 2 and k7.level(a, b, 1.0).all()


def test_k80_own_branch_is_the_general_form_to_the_bit():
    """at kappa == 1 — the only kappa fabs(kappa - 1) < 1e-20 lets through — the general form gives the bits of K80's own branch:
    its two expm1 take the same argument ((-2 bl) 2 / 3 == (-4 bl) / 3), (e1 - 2 e1)/4 == -e1/4, and (e1 + 2 e1)/4 rounds as
    3/4 e1 does (scaling by 4 is exact).  So no value tells whether the branch ran: a build without it computes the same
    matrices, and the device test can hold K80 at (1, 1) to the branch's form only (one value on the diagonal, one beside it)"""
    rng = np.random.default_rng(1)
    bl = np.concatenate([np.exp(rng.uniform(np.log(1e-320), np.log(1e4), 100000)), np.array(k7.BL), [5e-324]])
    kappa = 1.0
    e1, e2 = np.expm1(-4 * bl / (kappa + 2)), np.expm1(-2 * bl * (kappa + 1) / (kappa + 2))
    assert (e1 == e2).all()
    assert (1. + 3 / 4. * e1 == 1 + (e1 + 2 * e2) / 4).all() and (-e1 / 4 == (e1 - 2 * e2) / 4).all()
    for t in k7.BL:
        P = oracle_matrix("k80", k7.UNIFORM, (1.0, 1.0), t)
        e = float(np.expm1(-4 * t / 3))
        assert all(P[i, j] == (1 + (e + 2 * e) / 4 if i == j else (e - 2 * e) / 4) for i in range(4) for j in range(4)), t


# ------------------------------------------------------------------------------------------------ the seeds of the bound walks
def _configure(drv, data):
    s = k7.BOUND_SHAPE
    E.configure(drv, s["taxa"], s["windows"], s["R"], data, host=True)


@needs_ref
@pytest.mark.parametrize("model", k7.BOUND_MODELS)
def test_lower_bound_seed_comes_back_from_the_floor_and_rejects(model):
    """the seed of tests/test_gpu_closedform_edges.py's lower-bound walk of `model`: on the C driver with the reference's own
    likelihood some locus ends an iteration with a moved component inside [1e-5, 1.2e-5), none goes below 1e-5, and some
    proposal is rejected"""
    s = k7.BOUND_SHAPE
    data, which = k7.lower_bound_data(model)
    for d, w in zip(data, which):
        assert abs(d["freqs"].sum() - 1) < 1e-15 and (w[0] is None or (d["freqs"][w[0]] == k7.NEAR_FLOOR and w[0] != k7.FREQ_REF))
        assert w[1] is None or (d["exch"][w[1]] == k7.NEAR_FLOOR and w[1] != CF.TABLE[model][1])
    drv = CF.reference_driver(data, seed=k7.LOWER_SEEDS[model])
    _configure(drv, data)
    drv.initialize()
    hits = []
    for it in range(s["iters"]):
        drv.iterate()
        for i in range(s["nloci"]):
            f, q, _ = drv.get_subst_model(i)
            assert k7.floors_hold(model, f, q), (it, i, f, q)
            hits.extend((it, i, what) for what in k7.at_floor(model, (f, q), which[i]))
    p, a, _ = drv.counters()
    drv.close()
    print(f"[k7 host] lower bound {model}: {len(hits)} (iteration, locus, component) inside [1e-5, 1.2e-5); accepted {a} of {p}")
    assert hits and 0 < a < p, (hits, a, p)
    assert {h[2] for h in hits} == ({"freq"} if model == "f81" else {"entry"} if model == "k80" else {"freq", "entry"}), hits


@needs_ref
@pytest.mark.parametrize("model", k7.BOUND_MODELS)
def test_upper_bound_start_on_the_c_driver(model):
    """f = (.3, .3, .4 - 1e-9, 1e-9) and the reference entry at 1e-9, windows of 3.0: positive finite parameters, frequencies that
    sum to 1 within 4 ulp and finite likelihoods after every iteration; some locus leaves its start"""
    s = k7.BOUND_SHAPE
    data = k7.upper_bound_data(model)
    drv = CF.reference_driver(data, seed=k7.UPPER_SEED)
    _configure(drv, data)
    drv.initialize()
    for it in range(s["iters"]):
        drv.iterate()
        for i in range(s["nloci"]):
            f, q, a = drv.get_subst_model(i)
            assert min(f) > 0 and min(q) > 0 and np.isfinite(f).all() and np.isfinite(q).all(), (it, i, f, q)
            assert abs((f[0] + f[1] + f[2] + f[3]) - 1.0) <= 4 * 2.0 ** -52, (it, i, f)
            assert np.isfinite(drv.tree(i)["lnl"]), (it, i)
    moved = sum(list(drv.get_subst_model(i)[k]) != list(data[i][key]) for i in range(s["nloci"]) for k, key in ((0, "freqs"), (1, "exch")))
    drv.close()
    assert moved > 0
