"""Inputs of the substitution-parameter edge tests (tests/test_gpu_subst_edges.py on the device, tests/test_subst_edges_host.py
for what can be settled without one): the eigensystems at which eigen_sym_static's data-dependent branches turn, and the two
data sets that start the frequency / exchangeability moves at their reflection bounds.  Plain helper module, no fixtures."""
import numpy as np

import bpp_amd
from bpp_amd import synth

Q0 = (1.2, 3, .7, .9, 4, 1)
F0 = (.1, .2, .3, .4)
# (name, frequencies, exchangeabilities): repeated eigenvalues (JC / K80 / F81 / HKY shapes), frequencies at the moves' floor of
# 1e-5 and, for the reference component (v[ref] = sum - v[j] has no floor), below it; exchangeabilities at the floor and far above
EIGEN_CASES = [
    ("JC", (.25, .25, .25, .25), (1, 1, 1, 1, 1, 1)),
    ("K80-shaped", (.25, .25, .25, .25), (1, 4, 1, 1, 4, 1)),
    ("F81-shaped", F0, (1, 1, 1, 1, 1, 1)),
    ("HKY-shaped", F0, (1, 4, 1, 1, 4, 1)),
    ("one frequency 1e-5", (1e-5, .3, .3, .39999), Q0),
    ("two frequencies 1e-5", (1e-5, 1e-5, .5, .49998), Q0),
    ("reference frequency 1e-12", (.3, .3, .4 - 1e-12, 1e-12), Q0),
    ("q0 = 1e-5", F0, (1e-5, 3, .7, .9, 4, 1)),
    ("q0 = 1e3", F0, (1e3, 3, .7, .9, 4, 1)),
    ("last q = 1e-5", F0, (1.2, 3, .7, .9, 4, 1e-5)),
    ("five q at 1e-5", F0, (1e-5, 1e-5, 1e-5, 1e-5, 1e-5, 1)),
]
BRANCH_LENGTHS = (0.0, 1e-9, 0.01, 0.3, 2.0)
FLOOR = 1e-5                       # reflect(.., log 1e-5, log sum) of the moves (gsampler.hpp modes 6 / 7; locus.c:2819, 3248)
NEAR_FLOOR = 1.2e-5
FREQ_REF, Q_REF = 3, 1             # the components that take the remainder (T; the A<->G rate)


def with_model(data, freqs, exch, alpha):
    """the loci of a synth data set with their own substitution parameters (what the engine loci are made from)"""
    out = []
    for d, f, q, a in zip(data, freqs, exch, alpha):
        d = dict(d)
        d["freqs"], d["exch"] = np.array(f, dtype=float), np.array(q, dtype=float)
        d["rates"] = bpp_amd.compute_gamma_cats(a, a, d["rate_cats"])
        d["alpha"] = float(a)
        out.append(d)
    return out


def eigen_case_data(R=4):
    """one 4-tip GTR locus of 40 sites per edge eigensystem"""
    data = synth.make_dataset(len(EIGEN_CASES), 40, 4, "gtr", R, seed=57)
    return with_model(data, [c[1] for c in EIGEN_CASES], [c[2] for c in EIGEN_CASES], [0.7] * len(EIGEN_CASES))


GAMMA_SEED, GAMMA_FINETUNE, GAMMA_WINDOWS, GAMMA_ITERS = 43, (0.003, 0.005, 0.0004, 0.05), (1e-6, 1e-6, 0.05), 6


def gamma_grid_data(grid, R):
    """one 4-tip GTR locus of 40 sites per grid alpha, R categories"""
    base = synth.make_dataset(len(grid), 40, 4, "gtr", R, seed=51)
    return with_model(base, [d["freqs"] for d in base], [d["exch"] for d in base], grid)


BOUND_SHAPE = dict(nloci=24, sites=60, taxa=8, R=4, iters=6, windows=(3.0, 3.0, 0.8))
Q_MOVED = (0, 2, 3, 4, 5)
LOWER_SEED, UPPER_SEED, EIGEN_SEED = 29, 29, 47          # the samplers' seeds (chosen on the CPU: tests/test_subst_edges_host.py)


def lower_bound_data(seed=61):
    """every locus starts with one non-reference frequency and one non-reference exchangeability at 1.2e-5 (which ones: by
    locus number) -> (data, [(frequency index, exchangeability index)])"""
    s = BOUND_SHAPE
    data = synth.make_dataset(s["nloci"], s["sites"], s["taxa"], "gtr", s["R"], seed=seed)
    freqs, exch, which = [], [], []
    for i in range(s["nloci"]):
        jf, jq = i % 3, Q_MOVED[i % 5]
        f = np.array([0.3, 0.2, 0.2, 0.3])
        f[FREQ_REF] += f[jf] - NEAR_FLOOR; f[jf] = NEAR_FLOOR
        q = np.array([1, 2, 1, 0.5, 1.5, 1.0])
        q[jq] = NEAR_FLOOR
        freqs.append(f); exch.append(q); which.append((jf, jq))
    return with_model(data, freqs, exch, [0.5] * s["nloci"]), which


def upper_bound_data(ref=1e-9, seed=67):
    """every locus starts at f = (.3, .3, .4 - ref, ref): nearly every upward proposal of a frequency reflects at log(sum), and
    v[ref] = sum - exp(l_new) cancels"""
    s = BOUND_SHAPE
    data = synth.make_dataset(s["nloci"], s["sites"], s["taxa"], "gtr", s["R"], seed=seed)
    f = [.3, .3, .4 - ref, ref]
    return with_model(data, [f] * s["nloci"], [[1, 2, 1, 0.5, 1.5, 1.0]] * s["nloci"], [0.5] * s["nloci"])


def configure(drv, taxa, windows, R=None, data=None, host=False):
    """the uniform-window set-up of tests/test_gpu_gsampler.py's parameter-move test on a device sampler or a host driver"""
    parent, tau0, thetas = synth.species_tree_arrays(taxa)
    drv.set_species_tree(parent, tau0, thetas)
    drv.set_tau_prior(3.0, 3.0 / tau0[-1])
    drv.set_theta_prior(2.0, 1000.0, 0.001)
    drv.set_finetune(0.003, 0.005, 0.0008, 0.2)
    drv.set_subst_moves(*windows, 1.0, 1.0)
    for i, d in enumerate(data):
        if host:
            drv.set_subst_model(i, list(d["freqs"]), list(d["exch"]), d["alpha"], R)
        else:
            drv.set_subst_model(i, d["freqs"], d["exch"], d["alpha"])
    return parent, tau0, thetas


def at_floor(model, which):
    """a locus's moved components that sit in [1e-5, 1.2e-5): only a proposal reflected at (or landing next to) the floor puts
    one there after the start"""
    f, q, _ = model
    return [name for name, v in (("freq", f[which[0]]), ("exch", q[which[1]])) if FLOOR <= v < NEAR_FLOOR]
