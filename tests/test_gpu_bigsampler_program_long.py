"""The big-tree sampler with BPP's kernel and the program's moves after a longer run — no host driver alongside (the two
trajectories split on a last-bit log / sqrt after a few dozen iterations):

 * the state invariants of tests/test_gpu_state_invariants.py (check_state: tree, buffer indices, populations, MSC density,
   log-likelihood, root buffer, P-matrices, inner CLVs, scale counters against a from-scratch recompute on the CPU) on the
   24-tip loci with scalers and on the frogs loci, with that file's own bars;
 * usedata = 0: the marginals of every theta and of the root tau are their priors (the `big-4x6` case of
   tests/test_gpu_prior.py::test_all_loci_moves_leave_the_priors_with_several_sequences_per_species, its bars).

Measured on one MI355X (the columns of the table in tests/test_gpu_state_invariants.py):

  case                          iterations  loci   acc   lnl       root buffer  total     P ulps  P abs
  big, 24 tips, program's moves         50    12  0.44   0.0       0.0          0.0       0       1.1e-16
  big, frogs, program's moves           30     5  0.28   0.0       0.0          0.0       0       0.0

(logpr 0.0 in both.)  The prior run: the seven thetas' means 0.00186-0.00234 against 0.002 (at most 3.3 batch standard errors
off), sd ratios 0.91-1.05; the root tau's mean 0.00406 against 0.0045 (2.6 standard errors), sd ratio 0.81.
"""
import json
import os

import numpy as np
import pytest

import bpp_amd
from bpp_amd import synth, seqio
import tape
from test_gpu_state_invariants import grow, make
from test_gpu_prior import CASES, _batch_se

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_big_sampler_program_moves_on_24_tip_loci_with_scalers_state():
    """the data of tests/test_gpu_state_invariants.py::test_big_sampler_on_24_tip_loci_with_scalers"""
    eng = bpp_amd.Engine(0)
    rng = np.random.default_rng(5)
    stree = synth.species_tree_arrays(4, 0.004)
    parent, tau0, thetas = stree
    species = [k // 6 for k in range(24)]
    data = []
    for _ in range(12):
        left, right, times, root = synth.msc_start_tree(species, parent, tau0, thetas, rng)
        base = "".join(rng.choice(list("ACGT"), 200))
        seqs = ["".join(c if rng.random() > 0.04 else rng.choice(list("ACGT")) for c in base) for _ in range(24)]
        pats, w = bpp_amd.compress_site_patterns(seqs, True, True)
        data.append(dict(seqs=pats, weights=w, left=left, right=right, times=times, root=root, states=4, rate_cats=1, model="jc69", rates=np.ones(1)))
    sp = [species] * len(data)
    dev, loci = make(eng, data, stree, 3, "program", species=sp, prior=(2.0, 500.0, 0.001), finetune=(0.002, 0.003, 0.0004, 0.1),
                     loci=tape.make_engine_loci(eng, data, True))
    dev.initialize()
    assert dev.kind() == "big"
    grow("big-scalers-program", dev, (2, 50), tau0, thetas, data=data, species_parent=parent, loci=loci, tip_species=sp, scaling=True)
    assert dev.gibbs_counters()[0] > 0
    dev.close(); eng.close()


def test_big_sampler_program_moves_on_the_frogs_loci_state():
    """the data of tests/test_gpu_state_invariants.py::test_big_sampler_on_the_frogs_loci"""
    gold = json.load(open(os.path.join(G, "input_pipeline.json")))
    recs = seqio.load_dataset(os.path.join(G, "frogs", "frogs.txt"), os.path.join(G, "frogs", "frogs.Imap.txt"), gold["species"], [1, 1, 1, 1], model="jc69")
    eng = bpp_amd.Engine(0)
    parent = [4, 4, 5, 6, 5, 6, -1]
    tau0 = [0.0] * 4 + [0.01, 0.02, 0.03]
    thetas = [0.02] * 7
    rng = np.random.default_rng(9)
    data = []
    for r in recs:
        left, right, times, root = synth.msc_start_tree(r["species"], parent, tau0, thetas, rng)
        data.append(dict(seqs=r["seqs"], weights=r.get("weights", np.ones(len(r["seqs"][0]))), left=left, right=right, times=times, root=root,
                         states=4, rate_cats=1, model="jc69", rates=np.ones(1), diploid=r.get("diploid")))
    assert max(len(r["seqs"]) for r in recs) > 16 and all(d["diploid"] is not None for d in data)
    sp = [r["species"] for r in recs]
    dev, loci = make(eng, data, (parent, tau0, thetas), 8, "program", species=sp, tau_prior=(3.0, 100.0), prior=(3.0, 150.0, 0.003),
                     finetune=(0.004, 0.004, 0.002, 0.1), loci=[seqio.make_locus(eng, r) for r in recs])
    dev.initialize()
    assert dev.kind() == "big"
    grow("frogs-program", dev, (2, 30), tau0, thetas, data=data, species_parent=parent, loci=loci, tip_species=sp)
    assert dev.gibbs_counters()[0] > 0
    dev.close(); eng.close()


def test_the_program_s_moves_leave_the_priors_on_the_big_tree_sampler():
    """usedata = 0, 4 species x 6 sequences, two loci, all moves on: Gibbs thetas of tip populations, the re-draws inside the
    rubber band and the mixing step leave every theta's and the root tau's marginal at its gamma prior"""
    c = CASES["big-4x6"]
    samples, thin = 700, 2
    nsp = (len(c["parent"]) + 1) // 2
    tips = nsp * c["per"]
    species = [k // c["per"] for k in range(tips)]
    npop = len(c["parent"])
    a_th, b_th = 3.0, 3.0 / 0.002
    a_tau, b_tau = 4.0, 4.0 / c["tau"][-1]
    thetas = [a_th / b_th] * npop
    rng = np.random.default_rng(5)
    data = []
    for _ in range(2):
        left, right, times, root = synth.msc_start_tree(species, c["parent"], c["tau"], thetas, rng)
        pats, w = bpp_amd.compress_site_patterns(["ACGT"] * tips, True, True)
        data.append(dict(seqs=pats, weights=w, left=left, right=right, times=times, root=root, states=4, rate_cats=1, model="jc69", rates=np.ones(1)))
    eng = bpp_amd.Engine(0)
    eng.set_options(usedata=0, bfbeta=1.0)
    try:
        dev = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, data), data, seed=23)
        dev.set_species_tree(c["parent"], c["tau"], thetas)
        for i in range(len(data)):
            dev.set_tip_species(i, species)
        dev.set_tau_prior(a_tau, b_tau)
        dev.set_theta_prior(a_th, b_th, 0.002)
        dev.set_finetune(0.004, 0.004, 0.4 * c["tau"][-1], 0.5)
        dev.set_proposal_kernel(1)
        dev.set_program_moves(True, 0.1)
        dev.initialize()
        assert dev.kind() == "big"
        dev.iterate(600)
        S = []
        for _ in range(samples):
            dev.iterate(thin)
            S.append(dev.thetas() + dev.taus())
        S = np.array(S)
        for p in range(npop):
            x = S[:, p]
            print(f"[big-program prior] theta {p}: mean {x.mean():.6g} (prior {a_th / b_th:.6g}, batch se {_batch_se(x):.3g}), sd ratio {x.std() / (np.sqrt(a_th) / b_th):.3f}")
        x = S[:, 2 * npop - 1]
        print(f"[big-program prior] root tau: mean {x.mean():.6g} (prior {a_tau / b_tau:.6g}, batch se {_batch_se(x):.3g}), sd ratio {x.std() / (np.sqrt(a_tau) / b_tau):.3f}")
        for p in range(npop):
            x = S[:, p]
            assert abs(x.mean() - a_th / b_th) < 4.5 * _batch_se(x), (p, x.mean(), _batch_se(x))
            assert 0.75 < x.std() / (np.sqrt(a_th) / b_th) < 1.25, (p, x.std())
        x = S[:, 2 * npop - 1]
        assert abs(x.mean() - a_tau / b_tau) < 4.5 * _batch_se(x), (x.mean(), _batch_se(x))
        assert 0.8 < x.std() / (np.sqrt(a_tau) / b_tau) < 1.2
        g = dev.gibbs_counters()
        assert g[0] > samples
        dev.close()
    finally:
        eng.set_options(usedata=1, bfbeta=1.0)
        eng.close()
