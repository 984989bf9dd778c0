"""Inputs and the exact twin of the closed-form DNA models' edge tests (K7: csrc/kernels.hpp pmatrix_dna_closed, the reference's
locus.c:1981-2323) — tests/test_closedform_edges_host.py for what needs no GPU, tests/test_gpu_closedform_edges.py on the device.

EDGE_CASES x BL is the grid: frequencies from ordinary down to the moves' reflection floor of 1e-5 (and a reference frequency
below it), entries whose ratio kappa runs from 5e-13 to 2e12 and through K80's own branch at kappa == 1, branch length x rate from
0 and 1e-300 to 1e3.  exact_pmatrix evaluates the six forms as the reference writes them, in `decimal` at 60 digits from the exact
values of the doubles, and returns with every entry the sum S of the absolute values of its addends.  level() is the bar: 8 ulp,
or 5e-16 max(1, S) absolute — the project's PMAT_ULPS / PMAT_ATOL wherever S <= 1; beyond that scaled as tests/
test_gpu_subst_edges.py scales by max(1, |W||V|): two double evaluations that differ by an ulp in each expm1, or by a contraction,
differ by a few 2^-53 per addend.  Plain helper module, no fixtures."""
import decimal
from decimal import Decimal as D

import numpy as np

import bpp_amd
from bpp_amd import synth
import closedform as CF

PMAT_ULPS, PMAT_ATOL = 8, 5e-16
U53 = 2.0 ** -53
FLOOR, NEAR_FLOOR = 1e-5, 1.2e-5
BL = (0.0, 1e-300, 1e-9, 0.01, 0.3, 2.0, 50.0, 1e3)
EDGE_ALPHA = 0.05                                  # Gamma4 rates 5e-13, 1e-6, 5e-3 and 4: lengths x rates from denormal (1e-313) to 4e3
TINY_ALPHA = 0.005                                 # Gamma4 rates 2e-121, 7e-61, 2e-25 and 4: 1e-300 x rate underflows to 0

UNIFORM = (.25, .25, .25, .25)
# (name, A, C, G, T)
FREQS = [
    ("uniform", UNIFORM),
    ("plain", (.1, .2, .3, .4)),
    ("A=1e-5", (1e-5, .3, .3, .39999)),
    ("R=2e-5", (1e-5, .5, 1e-5, .49998)),
    ("C=1e-5,T=1e-12", (.5, 1e-5, .49999 - 1e-12, 1e-12)),
    ("three=1e-5", (1e-5, 1e-5, 1e-5, .99997)),
]
FREQS_T92 = FREQS + [("GC=2e-5", (.5, .49998, 1e-5, 1e-5)), ("GC=1-2e-5", (1e-5, 1e-5, .5, .49998))]
# (q0, q1) of the two-entry models: K80 / HKY read kappa = q1/q0, T92 / F84 kappa = q0/q1 — both ends are small in one, large in the other
TWO = [
    ("1:1", (1.0, 1.0)),
    ("1:1+ulp", (1.0, 1.0 + 2.0 ** -52)),
    ("1:4", (1.0, 4.0)),
    ("q0=1e-5", (1e-5, 2 - 1e-5)),
    ("q1=1e-5", (2 - 1e-5, 1e-5)),
    ("q1=1e-12", (2 - 1e-12, 1e-12)),
]
THREE = [
    ("1:2:1", (1.0, 2.0, 1.0)),
    ("q0=1e-5", (1e-5, 2.0, 1.0)),
    ("q1=1e-5", (1.0, 1e-5, 1.0)),
    ("q0=q1=1e-5", (1e-5, 1e-5, 1.0)),
    ("q2=1e-12", (1.0, 2.0, 1e-12)),
]


def _cases():
    out = []
    for qn, q in TWO:
        out.append((f"k80 {qn}", "k80", UNIFORM, q))
    for fn, f in FREQS:
        out.append((f"f81 {fn}", "f81", f, ()))
    for m, fl, ql in (("hky", FREQS, TWO), ("t92", FREQS_T92, TWO), ("tn93", FREQS, THREE), ("f84", FREQS, TWO)):
        for fn, f in fl:
            for qn, q in ql:
                out.append((f"{m} {fn} {qn}", m, f, q))
    return out


EDGE_CASES = _cases()                              # (name, model, frequencies A, C, G, T, the model's entries)
K80_BRANCH = "k80 1:1"                             # fabs(kappa - 1) < 1e-20: only kappa == 1 takes it


def padded(q):
    """the model's entries padded to six with ones, as closedform.with_model does"""
    return np.array(list(q) + [1.0] * (6 - len(q)), dtype=float)


def cases_of(model):
    return [c for c in EDGE_CASES if c[1] == model]


# ------------------------------------------------------------------------------------------------ the exact twin
_CTX = decimal.Context(prec=60, Emin=-10 ** 17, Emax=10 ** 17)
# T92 as the reference writes it: row i of the written matrix is the row of state T92_ROW[i] of a reversible matrix with the
# stationary vector ((1-GC)/2, GC/2, GC/2, (1-GC)/2) (the "1 +" stands at column T92_ROW[i]); parity with that is the contract
T92_ROW = (3, 1, 0, 2)


def _exp(x):
    """exp(x) with 60 digits left in exp(x) - 1: the working precision grows with the zeros behind the point"""
    if x == 0:
        return D(1)
    extra = max(0, -x.adjusted())
    c = decimal.Context(prec=60 + extra, Emin=-10 ** 17, Emax=10 ** 17)
    return c.exp(x)


def _expm1(x):
    if x == 0:
        return D(0)
    extra = max(0, -x.adjusted())
    c = decimal.Context(prec=60 + extra, Emin=-10 ** 17, Emax=10 ** 17)
    return c.subtract(c.exp(x), D(1))


def exact_addends(model, f, q, bl):
    """the 4 x 4 lists of addends of P(bl) by the reference's closed form of `model` (a name), every operation at 60 digits"""
    decimal.setcontext(_CTX)
    f = [D(float(x)) for x in f]
    q = [D(float(x)) for x in q]
    bl = D(float(bl))
    one, two, four = D(1), D(2), D(4)
    P = [[None] * 4 for _ in range(4)]
    if model == "k80":
        kappa = q[1] / q[0]
        e1 = _expm1(-4 * bl / (kappa + 2))
        if abs(kappa - 1) < D("1e-20"):
            for i in range(16):
                P[i >> 2][i & 3] = [one, D(3) / four * e1] if (i >> 2) == (i & 3) else [-e1 / four]
        else:
            e2 = _expm1(-2 * bl * (kappa + 1) / (kappa + 2))
            for i in range(16):
                r, c = i >> 2, i & 3
                P[r][c] = [one, e1 / four, two * e2 / four] if r == c else [e1 / four, -two * e2 / four] if (r ^ c) == 2 else [-e1 / four]
    elif model == "f81":
        beta = one
        for j in range(4):
            beta -= f[j] * f[j]
        beta = one / beta
        e, em1 = _exp(-beta * bl), _expm1(-beta * bl)
        for i in range(16):
            r, c = i >> 2, i & 3
            P[r][c] = [e, -f[c] * em1] if r == c else [-f[c] * em1]
    elif model == "t92":
        GC = f[3] + f[2]
        e1 = _expm1(-bl)
        e2 = _expm1(-(q[0] / q[1] + 1) * bl / two)
        a, g = [-(1 - GC) / two * e1], [-GC / two * e1]
        x = [GC / two * e1, -GC * e2]
        y = [(1 - GC) / two * e1, -(1 - GC) * e2]
        dx = [one, D("0.5") * (1 - GC) * e1, GC * e2]
        dy = [one, GC / two * e1, (1 - GC) * e2]
        P = [[a, x, g, dx], [a, dy, g, y], [dx, g, x, a], [y, g, dy, a]]
    else:
        A, C, G, T = f
        Y, R = T + C, A + G
        if model == "hky":
            kappa = q[1] / q[0]
            mr = one / (2 * T * C * kappa + 2 * A * G * kappa + 2 * Y * R)
            bt = bl * mr
            a1t = a2t = kappa * bt
        elif model == "f84":
            kappa = q[0] / q[1]
            mr = one / (2 * T * C * kappa + 2 * A * G * kappa + 2 * Y * R)
            bt = bl * mr
            a1t, a2t = (1 + kappa / Y) * bt, (1 + kappa / R) * bt
        else:
            assert model == "tn93", model
            mr = one / (2 * T * C * q[0] + 2 * A * G * q[1] + 2 * Y * R)
            bt = bl * mr
            a1t, a2t = (q[0] / q[2]) * bt, (q[1] / q[2]) * bt
        e1, e2, e3 = _expm1(-bt), _expm1(-(R * a2t + Y * bt)), _expm1(-(Y * a1t + R * bt))
        P[0] = [[one, Y * A / R * e1, G / R * e2], [-C * e1], [Y * G / R * e1, -(G / R * e2)], [-T * e1]]
        P[1] = [[-A * e1], [one, R * C * e1 / Y, T * e3 / Y], [-G * e1], [R * e1 * T / Y, -(e3 * T / Y)]]
        P[2] = [[Y * A / R * e1, -(A / R * e2)], [-C * e1], [one, Y * G / R * e1, A / R * e2], [-T * e1]]
        P[3] = [[-A * e1], [R * e1 * C / Y, -(e3 * C / Y)], [-G * e1], [one, R * T * e1 / Y, C * e3 / Y]]
    return P


def exact_pmatrix(model, f, q, bl):
    """-> (P, S): the exact value of the reference's form at these doubles and, per entry, the sum of |addends|, as 4 x 4 lists
    of Decimal"""
    add = exact_addends(model, f, q, bl)
    decimal.setcontext(_CTX)
    return ([[sum(a, D(0)) for a in row] for row in add], [[sum((abs(v) for v in a), D(0)) for a in row] for row in add])


def stationary(model, f):
    """the stationary vector the form implies, as Decimals: the frequencies; T92: ((1-GC)/2, GC/2, GC/2, (1-GC)/2), GC = f[3] + f[2]"""
    decimal.setcontext(_CTX)
    f = [D(float(x)) for x in f]
    if model == "k80":
        return [D("0.25")] * 4
    if model == "t92":
        GC = f[3] + f[2]
        return [(1 - GC) / 2, GC / 2, GC / 2, (1 - GC) / 2]
    return f


def rows_by_state(model, P):
    """the matrix with its rows in the order of the states: the written one for every model but T92 (T92_ROW)"""
    if model != "t92":
        return P
    out = [None] * 4
    for i, s in enumerate(T92_ROW):
        out[s] = P[i]
    return out


# ------------------------------------------------------------------------------------------------ the bar
def as_float(P):
    return np.array([[float(x) for x in row] for row in P])


def ulps(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.maximum(np.spacing(np.maximum(np.abs(a), np.abs(b))), 1e-320)


def level(got, want, S):
    """entrywise: within 8 ulp of the target, or within 5e-16 max(1, S) absolute -> boolean array"""
    got, want = np.asarray(got, float), np.asarray(want, float)
    return (ulps(got, want) <= PMAT_ULPS) | (np.abs(got - want) <= PMAT_ATOL * np.maximum(1.0, S))


def distance(got, want, S):
    """entrywise |got - want| in units of 2^-53 max(1, S); the absolute bar is 5e-16 / 2^-53 = 4.5 of these"""
    return np.abs(np.asarray(got, float) - np.asarray(want, float)) / (U53 * np.maximum(1.0, S))


def exact_distance(model, f, q, bl, got):
    """a double matrix against the exact twin -> (entrywise level, entrywise distance), the difference taken at 60 digits"""
    P, S = exact_pmatrix(model, f, q, bl)
    got = np.asarray(got, float)
    Sf = as_float(S)
    diff = np.array([[float(abs(D(float(got[i, j])) - P[i][j])) for j in range(4)] for i in range(4)])
    want = as_float(P)
    ok = (ulps(got, want) <= PMAT_ULPS) | (diff <= PMAT_ATOL * np.maximum(1.0, Sf))
    return ok, diff / (U53 * np.maximum(1.0, Sf))


_S = {}


def addend_sums(model, f, q, bl):
    """S of the exact twin as doubles, kept per (model, f, q, bl)"""
    key = (model, tuple(float(x) for x in f), tuple(float(x) for x in q), float(bl))
    if key not in _S:
        _S[key] = as_float(exact_pmatrix(model, f, q, bl)[1])
    return _S[key]


# ------------------------------------------------------------------------------------------------ data sets
_DATA = {}


def edge_data(R, alpha=EDGE_ALPHA):
    """one 4-tip locus of 40 sites per edge case, declared with the case's model and values, R categories (rates of `alpha`)"""
    if (R, alpha) not in _DATA:
        base = synth.make_dataset(len(EDGE_CASES), 40, 4, "gtr", R, seed=71)
        out = []
        for d, (name, model, f, q) in zip(base, EDGE_CASES):
            d = dict(d, model=model, freqs=np.array(f, dtype=float), exch=padded(q), case=name, alpha=alpha,
                     rates=np.asarray(bpp_amd.compute_gamma_cats(alpha, alpha, R)) if R > 1 else np.ones(1))
            out.append(d)
        _DATA[(R, alpha)] = out
    return _DATA[(R, alpha)]


def scaled(d, factor):
    """the locus with every node age x factor"""
    return dict(d, times=[float(t) * factor for t in d["times"]])


# ------------------------------------------------------------------------------------------------ the moves' bounds
BOUND_SHAPE = dict(nloci=24, sites=60, taxa=8, R=4, iters=6, windows=(3.0, 3.0, 0.8))
BOUND_MODELS = ("k80", "f81", "hky", "t92", "tn93", "f84")          # (K80: its entry alone moves)
FREQ_REF = 3
# the samplers' seeds, chosen on the CPU (tests/test_closedform_edges_host.py): with them some locus of the model ends an
# iteration with a moved component inside [1e-5, 1.2e-5), and some proposal is rejected
LOWER_SEEDS = {"k80": 29, "f81": 29, "hky": 29, "t92": 29, "tn93": 29, "f84": 29}
UPPER_SEED = 29


def moved_entries(model):
    return CF.TABLE[model][2]


def lower_bound_data(model, seed=61):
    """24 loci of `model`: one non-reference frequency (which: by locus number; K80: none) and the model's moved entry (TN93: one of its two,
    by locus number) start at 1.2e-5; the reference entry keeps the entries' sum at 2 (TN93: q2 = 1)
    -> (data, [(frequency index, entry index or None)])"""
    s = BOUND_SHAPE
    base = synth.make_dataset(s["nloci"], s["sites"], s["taxa"], "gtr", s["R"], seed=seed)
    out, which = [], []
    for i, d in enumerate(base):
        jf = i % 3 if model != "k80" else None
        f = np.array([0.3, 0.2, 0.2, 0.3]) if model != "k80" else np.full(4, 0.25)
        if jf is not None:
            f[FREQ_REF] += f[jf] - NEAR_FLOOR; f[jf] = NEAR_FLOOR
        mv = moved_entries(model)
        jq = mv[i % len(mv)] if mv else None
        if model == "tn93":
            q = [1.0, 2.0, 1.0]; q[jq] = NEAR_FLOOR
        elif model == "f81":
            q = []
        else:
            q = [NEAR_FLOOR, 2 - NEAR_FLOOR]
        out.append(dict(d, model=model, freqs=f, exch=padded(q), alpha=0.5, rates=np.asarray(bpp_amd.compute_gamma_cats(0.5, 0.5, s["R"]))))
        which.append((jf, jq))
    return out, which


def upper_bound_data(model, ref=1e-9, seed=67):
    """24 loci of `model` at f = (.3, .3, .4 - ref, ref) with the reference entry at ref: nearly every upward proposal reflects at
    log(sum), and v[ref] = sum - exp(l_new) cancels"""
    s = BOUND_SHAPE
    base = synth.make_dataset(s["nloci"], s["sites"], s["taxa"], "gtr", s["R"], seed=seed)
    f = np.array([.3, .3, .4 - ref, ref]) if model != "k80" else np.full(4, 0.25)
    q = [] if model == "f81" else [1.0, 2.0, ref] if model == "tn93" else [2 - ref, ref]
    return [dict(d, model=model, freqs=f.copy(), exch=padded(q), alpha=0.5, rates=np.asarray(bpp_amd.compute_gamma_cats(0.5, 0.5, s["R"])))
            for d in base]


def bound_case(data):
    from bpp_amd import synth as sy
    return dict(data=data, species=None, stree=sy.species_tree_arrays(BOUND_SHAPE["taxa"]), model="gtr")


def at_floor(model, fq, which):
    """the locus's moved components inside [1e-5, 1.2e-5)"""
    f, q = fq[0], fq[1]
    vals = ([("freq", f[which[0]])] if which[0] is not None else []) + ([("entry", q[which[1]])] if which[1] is not None else [])
    return [name for name, v in vals if FLOOR <= v < NEAR_FLOOR]


def floors_hold(model, f, q):
    lo = FLOOR * (1 - 2.0 ** -52)
    return min(f[:3]) >= lo and all(q[j] >= lo for j in moved_entries(model))


# ------------------------------------------------------------------------------------------------ the batched routes
S17 = [0, 0, 0] + [k // 2 for k in range(2, 16)]          # 17 tips on 8 species (tests/test_gpu_closedform.py's layout)
SCALES = (1e-6, 1.0, 1e2)                                 # of the start trees' ages: lengths x rates from 1e-22 to 2
EXTRA_CASE = "f84 R=2e-5 q1=1e-5"                         # what the added loci are declared as: F84, both purines at the floor
# name -> (categories, scale buffers, listed against the slot order, the added locus (tips, patterns) or None, what plan_build
# (csrc/engine.hip) makes of it).  Every edge locus has 4 tips and at most 8 patterns.
ROUTES = {
    "klane-v3":    (4, False, False, None,      "step_s4_klane_v3_kernel + pmatrix_s4_dense_kernel"),
    "klane-v2":    (4, False, False, (17, 12),  "step_s4_klane_v2_kernel + pmatrix_s4_dense_kernel"),
    "klane-128":   (4, False, True,  None,      "step_s4_klane_kernel<128>"),
    "klane-256":   (4, False, True,  (4, 40),   "step_s4_klane_kernel<256>"),
    "fused-64-1":  (1, False, False, (4, 40),   "step_s4_fused_kernel<64, 1>"),
    "fused-256-1": (1, False, False, (4, 70),   "step_s4_fused_kernel<256, 1>"),
    "fused-64-4":  (4, True,  False, (4, 40),   "step_s4_fused_kernel<64, 4>"),
    "fused-256-4": (4, True,  False, (4, 70),   "step_s4_fused_kernel<256, 4>"),
    "fused-64-0":  (3, True,  False, (4, 40),   "step_s4_fused_kernel<64, 0>"),
    "fused-256-0": (3, True,  False, (4, 70),   "step_s4_fused_kernel<256, 0>"),
    "unfused":     (4, False, False, (4, 257),  "pmatrix_s4_kernel + partials_lnl_s4_kernel"),
}
_ROUTE_DATA = {}


def extra_locus(tips, npat, R):
    """one locus of exactly `npat` patterns (tests/shapes.py: ambiguity codes give a 4-tip locus enough distinct columns),
    declared as EXTRA_CASE with the edge sets' rates"""
    import shapes
    if tips == 17:
        d = shapes.shaped_locus(S17, synth.species_tree_arrays(8), npat, model="gtr", rate_cats=R, rng=np.random.default_rng(73))
    else:
        d = shapes.shaped_locus(list(range(tips)), synth.species_tree_arrays(tips), npat, model="gtr", rate_cats=R, rng=np.random.default_rng(74))
    name, model, f, q = next(c for c in EDGE_CASES if c[0] == EXTRA_CASE)
    return dict(d, model=model, freqs=np.array(f, dtype=float), exch=padded(q), case=f"{tips} tips, {npat} patterns: {name}", alpha=EDGE_ALPHA,
                rates=np.asarray(bpp_amd.compute_gamma_cats(EDGE_ALPHA, EDGE_ALPHA, R)) if R > 1 else np.ones(1))


def route_data(route):
    """the loci of a route: every edge locus at each of SCALES, then the added locus (unscaled)"""
    if route not in _ROUTE_DATA:
        R, _, _, extra, _ = ROUTES[route]
        data = [scaled(d, s) for s in SCALES for d in edge_data(R)]
        if extra is not None:
            data.append(extra_locus(extra[0], extra[1], R))
        _ROUTE_DATA[route] = data
    return _ROUTE_DATA[route]


def route_of(data, scaling, reverse):
    """plan_build's own conditions (csrc/engine.hip), worked out on the host -> the kernel a plan of these loci launches"""
    maxnp = max(len(d["weights"]) for d in data)
    if maxnp > 256:
        return "pmatrix_s4_kernel + partials_lnl_s4_kernel"
    cats = [d["rate_cats"] for d in data]
    klane = min(cats) > 1 and not scaling and max(len(d["weights"]) * d["rate_cats"] for d in data) <= 256
    if klane:
        maxlanes = max(len(d["weights"]) * d["rate_cats"] for d in data)
        if reverse:
            return f"step_s4_klane_kernel<{128 if maxlanes <= 128 else 256}>"
        maxops = max(len(d["seqs"]) - 1 for d in data)
        return ("step_s4_klane_v3_kernel" if 1 + max(maxops, 3) <= 16 else "step_s4_klane_v2_kernel") + " + pmatrix_s4_dense_kernel"
    BS = 256 if maxnp <= 16 else 64 if maxnp <= 64 else 256
    RT = 1 if max(cats) == 1 else 4 if min(cats) == max(cats) == 4 else 0
    return f"step_s4_fused_kernel<{BS}, {RT}>"
