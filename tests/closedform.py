"""Helpers of the closed-form DNA models' parameter-move tests (K80, F81, HKY, T92, TN93, F84 next to GTR; the reference's
counts locus.c:906-952, its frequency move :2782, the reference entries :3197-3229, the Dirichlet prior on the exchangeabilities
:3190, 3301-3304): a00_set_subst_kind and a00_set_qrates_prior bound on hostdrv.lib(), loci of any DNA model for the engine
and for the reference's locus API (tape.make_engine_loci and tape.ref_locus_for know jc69 and gtr only), the step table, the
closed form of the prior's term, the set-up of a trajectory pair.  Plain module, no fixtures."""
import ctypes as C
import math

import numpy as np

import bpp_amd
import hostdrv
import locusrates as LR
import oraclelib as O

MODELS = dict(O.DNA_MODELS)                                   # name -> BPA_DNA_MODEL_*
CLOSED = ("k80", "f81", "hky", "t92", "tn93", "f84")
# the issue's table, written out by hand: name -> (exchangeability entries, reference entry, entries the steps move, frequency steps)
TABLE = {
    "k80":  (2, 1, (0,), 0),
    "f81":  (0, None, (), 3),
    "hky":  (2, 1, (0,), 3),
    "t92":  (2, 1, (0,), 3),
    "f84":  (2, 1, (0,), 3),
    "tn93": (3, 2, (0, 1), 3),
    "gtr":  (6, 1, (0, 2, 3, 4, 5), 3),
}
PROGRAM_PRIOR = (2.0, 4.0, 2.0, 2.0, 4.0, 2.0)                # gtr_alpha of propose_qrates
FLAT_PRIOR = (1.0,)*6


def steps_of(models):
    """(frequency steps, exchangeability steps) an iteration runs for loci of these models: the loci's maximum"""
    return max(TABLE[m][3] for m in models), max(len(TABLE[m][2]) for m in models)


def proposals_of(models, rate_cats):
    """parameter proposals of one iteration: every locus its model's steps, + the alpha step with several categories"""
    return sum(TABLE[m][3] + len(TABLE[m][2]) + (1 if r > 1 else 0) for m, r in zip(models, rate_cats))


def lib():
    L = hostdrv.lib()
    if not getattr(L, "_closedform", False):
        L.a00_set_subst_kind.argtypes = [C.c_void_p, C.c_uint, C.c_int]
        L.a00_set_subst_kind.restype = C.c_int
        L.a00_set_qrates_prior.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.a00_set_qrates_prior.restype = C.c_int
        L._closedform = True
    return L


class KindDriver:
    """a hostdrv.Driver (or a wrapper of one) with the two new calls; set_qrates_prior under bpp_amd.Sampler's name"""

    def __init__(self, drv):
        self.drv = drv

    def __getattr__(self, name):
        return getattr(self.drv, name)

    def try_set_subst_kind(self, i, model):
        return bool(lib().a00_set_subst_kind(self.drv.h, i, MODELS.get(model, model)))

    def set_subst_kind(self, i, model):
        assert self.try_set_subst_kind(i, model), "a00_set_subst_kind refused"

    def try_set_qrates_prior(self, a):
        return bool(lib().a00_set_qrates_prior(self.drv.h, (C.c_double*6)(*[float(x) for x in a])))

    def set_qrates_prior(self, a):
        assert self.try_set_qrates_prior(a), "a00_set_qrates_prior refused"


# ---- loci of any DNA model
def with_model(data, models, kappa=2.0):
    """the loci of a data set (made as gtr: their columns are what they are) declared as `models` (one name, or one per locus):
    K80 gets equal frequencies, the exchangeabilities start at the model's own entries for a ratio of kappa (TN93: kappa and
    0.8 kappa), padded to six with ones; gtr keeps its own"""
    from bpp_amd import synth
    if isinstance(models, str):
        models = [models]*len(data)
    out = []
    for d, m in zip(data, models):
        d = dict(d, model=m)
        if m != "gtr":
            d["freqs"] = np.full(4, 0.25) if m == "k80" else np.array(d["freqs"], dtype=float)
            d["exch"] = synth.closed_form_rates(m, kappa, d["freqs"])[0]
        out.append(d)
    return out


def recat(d, rate_cats, alpha=0.5):
    """the locus with another number of rate categories"""
    return dict(d, rate_cats=rate_cats, rates=bpp_amd.compute_gamma_cats(alpha, alpha, rate_cats) if rate_cats > 1 else np.ones(1))


def make_engine_loci(engine, data, scaling=False):
    """tape.make_engine_loci for loci of any DNA model"""
    loci = []
    for d in data:
        R = d["rate_cats"]
        tips, sites = len(d["seqs"]), len(d["seqs"][0])
        inner, edges = tips - 1, 2*tips - 2
        loc = bpp_amd.Locus(engine, bpp_amd.DATA_DNA, MODELS[d["model"]], tips, 2*inner, 4, sites, 1, 2*edges, R, 2*inner if scaling else 0)
        for i, s in enumerate(d["seqs"]):
            loc.set_tip_states(i, s)
        loc.set_pattern_weights(d["weights"])
        if d["model"] != "jc69":
            loc.set_frequencies(0, d["freqs"])
            loc.set_subst_params(0, d["exch"])
        loc.set_category_rates(d["rates"])
        loci.append(loc)
    return loci


def ref_locus_for(d, scaling=False):
    rl = O.RefLocus(4, d["rate_cats"], d["seqs"], d["weights"], model=d["model"], freqs=d["freqs"], qrates=d["exch"],
                    rates=d["rates"], scaling=scaling)
    rl.set_tree(d["left"], d["right"], d["times"], d["root"])
    return rl


def reference_driver(data, seed=1, scaling=False, kinds=True):
    """the host driver on the REAL reference's locus API, every locus of its own model (kinds: tell the driver)"""
    rls = [ref_locus_for(d, scaling) for d in data]
    arr = (C.c_void_p*len(rls))(*[rl.h for rl in rls])
    drv = hostdrv.Driver(data, C.cast(O.ref().ref_backend_eval, C.c_void_p), C.cast(arr, C.c_void_p), seed, scaling)
    drv._keep = (rls, arr)
    drv.set_param_backend(C.cast(O.ref().ref_backend_params, C.c_void_p))
    drv = KindDriver(LR.RateDriver(drv))
    if kinds:
        for i, d in enumerate(data):
            drv.set_subst_kind(i, d["model"])
    return drv


def hip_driver(eng, data, seed=1, scaling=False):
    """the host driver on libbpp_amd.so with loci of its own, every locus's model declared"""
    drv = KindDriver(LR.RateDriver(hostdrv.hip_driver(eng, make_engine_loci(eng, data, scaling), data, seed=seed, scaling=scaling)))
    for i, d in enumerate(data):
        drv.set_subst_kind(i, d["model"])
    return drv


def configure(drv, c, moves, host, prior=None, windows=(0.3, 0.4, 0.8)):
    """locusrates.configure's trajectory set-up with the three parameter moves on (no rate moves), then the windows and the
    prior on the exchangeabilities (None: the call is not made)"""
    LR.configure(drv, c, moves, host, subst=True, ft=None)
    drv.set_subst_moves(*windows, 1.0, 1.0)
    if prior is not None:
        drv.set_qrates_prior(prior)


# ---- the posterior of the unmodified program on HKY+Gamma4 data (tests/golden/hky_posterior.json, make_golden_hky.py)
GOLD_POP = {"A,B": 4, "A,B,C": 5, "A,B,C,D": 6}               # the inner populations in species_tree_arrays(4)'s order
_GOLD = {}


def gold():
    import json
    import os
    if "g" not in _GOLD:
        _GOLD["g"] = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hky_posterior.json")))
    return _GOLD["g"]


def gold_data():
    """the golden's alignments, every locus at BPP's start values (equal frequencies and rates, alpha at its prior mean)"""
    from bpp_amd import synth
    c = gold()["config"]
    data = synth.make_dataset(c["nloci"], c["sites"], c["taxa"], "hky", c["rate_cats"], seed=c["seed"], theta=c["theta"], kappa=c["kappa"])
    a0 = c["alpha_prior"][0]/c["alpha_prior"][1]
    for d in data:
        d["freqs"] = np.full(4, 0.25); d["exch"] = np.ones(6)
        d["rates"] = np.asarray(bpp_amd.compute_gamma_cats(a0, a0, c["rate_cats"]))
    return data


def gold_setup(drv, data, host, prior):
    """the golden's priors; uniform-window step lengths of this project's choosing (any widths sample the same posterior)"""
    from bpp_amd import synth
    c = gold()["config"]
    parent, tau, thetas = synth.species_tree_arrays(c["taxa"], c["theta"])
    drv.set_species_tree(parent, tau, thetas)
    drv.set_tau_prior(*c["tau_prior"])
    drv.set_theta_prior(c["theta_prior"][0], c["theta_prior"][1], 0.004)
    drv.set_finetune(0.004, 0.004, 0.0012, 0.2)
    a0 = c["alpha_prior"][0]/c["alpha_prior"][1]
    for i in range(len(data)):
        if host:
            drv.set_subst_model(i, [0.25]*4, [1.0]*6, a0, c["rate_cats"])
        else:
            drv.set_subst_model(i, [0.25]*4, [1.0]*6, a0)
    drv.set_subst_moves(0.5, 1.5, 1.2, c["alpha_prior"][0], c["alpha_prior"][1])
    if prior is not None:
        drv.set_qrates_prior(prior)


def gold_row(thetas, taus, lnl, qrates):
    """one sample in the golden's columns: thetas and taus of the inner populations, lnL, every locus's log kappa = log(q1/q0)"""
    row = {}
    for label, p in GOLD_POP.items():
        row["theta:" + label] = thetas[p]; row["tau:" + label] = taus[p]
    row["lnL"] = lnl
    for i, q in enumerate(qrates):
        row[f"logkappa:{i}"] = math.log(q[1]/q[0])
    return row


def gold_compare(rows, tol_mean=0.3, tol_sd=0.25, only=None):
    """the project's bars: mean within 0.3 sd, sd within 0.25 sd of the program's, per quantity -> the misses (empty: all hold)
    and the largest distances seen, in the program's sd"""
    misses, worst = [], [0.0, 0.0]
    for name, ref in gold()["posterior"].items():
        parts = name.split(":")
        key = name if parts[0] in ("lnL", "logkappa") else parts[0] + ":" + parts[2]
        if only is not None and not key.startswith(only):
            continue
        x = np.array([r[key] for r in rows])
        dm, ds = abs(x.mean() - ref["mean"])/ref["sd"], abs(x.std() - ref["sd"])/ref["sd"]
        worst = [max(worst[0], dm), max(worst[1], ds)]
        if not (dm < tol_mean and ds < tol_sd):
            misses.append((name, float(x.mean()), float(x.std()), ref["mean"], ref["sd"]))
    return misses, worst


# ---- the prior's term, from the reference's statements (locus.c:3301-3304)
def qrates_prior_lnratio(a, j, ref, qj_old, qj_new, qref_old, qref_new):
    return (a[j] - 1.0)*(math.log(qj_new) - math.log(qj_old)) + (a[ref] - 1.0)*math.log(qref_new/qref_old)


def untouched(model, q_start, q_now):
    """the entries the model does not have are == their starting values"""
    n = TABLE[model][0]
    return all(float(q_now[k]) == float(q_start[k]) for k in range(n, 6))


def conserved(model, f_start, q_start, f_now, q_now):
    """sum of the frequencies and q_j + q_ref per moved entry... the moves conserve the SUM of all entries that move against one
    reference: the frequencies' total, and the total of the model's exchangeability entries"""
    n = TABLE[model][0]
    df = abs(float(np.sum(f_now)) - float(np.sum(f_start)))
    dq = abs(float(np.sum(q_now[:n])) - float(np.sum(q_start[:n]))) if n else 0.0
    return df, dq
