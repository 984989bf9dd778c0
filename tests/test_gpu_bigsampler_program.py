"""BPP's own iteration on the big-tree device sampler (csrc/bigsampler.hpp: big_step_kernel<true> — the reference's generator,
Bactrian-Laplace windows and acceptance rule in the per-locus proposals; THETA by the metropolized Gibbs draw, the thetas
re-drawn inside the rubber band and the mixing step, decided on the device by gsm::gdec_kernel from the loci's sums):

 * the trajectory of the C host driver with a00_set_proposal_kernel(BPP) + a00_set_program_moves on the same library, on
   loci the big-tree sampler alone runs (24 tips with scalers, the frogs' unphased diploids) and on small loci forced onto it;
 * what it refuses: BPP's kernel without the program's moves or without a theta prior;
 * the burn-in's step-length rule (bpa_sampler_adapt_finetune / bpa_sampler_burnin) on its move-type counters.
"""
import json
import os

import numpy as np
import pytest

import bpp_amd
from bpp_amd import synth, seqio
import hostdrv
import tape
from test_gpu_gsampler import walk
from test_gpu_host_driver import _msc_start_tree

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _program(drv):
    drv.set_proposal_kernel(1)
    drv.set_program_moves(True, 0.3)


def _finish(host, dev, tau0, thetas, taus_moved=True):
    assert dev.kind() == "big"
    # (the Gibbs draws move thetas in every iteration; two iterations of a handful of loci can reject every rubber band and
    #  the mixing step on both sides alike)
    assert dev.thetas() != list(thetas) and (not taus_moved or dev.taus() != list(tau0))
    gh, gd = host.gibbs_counters(), dev.gibbs_counters()
    assert tuple(gd) == tuple(gh) and gd[0] > 0, (gd, gh)


@pytest.mark.parametrize("taxa,model,R,nloci,iters,scaling", [(4, "jc69", 1, 150, 5, False), (8, "gtr", 4, 30, 3, False), (8, "jc69", 1, 30, 3, True)])
def test_big_sampler_program_moves_forced_on_small_loci_equals_host_driver(taxa, model, R, nloci, iters, scaling):
    """the shapes, priors and step lengths of test_gpu_bigsampler.py::test_big_sampler_forced_on_small_loci_equals_host_driver"""
    eng = bpp_amd.Engine(0)
    data = synth.make_dataset(nloci, 300, taxa, model, R, seed=19)
    host = hostdrv.hip_driver(eng, tape.make_engine_loci(eng, data, scaling), data, seed=29, scaling=scaling)
    dev = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, data, scaling), data, seed=29, implementation="big")
    parent, tau0, thetas = synth.species_tree_arrays(taxa)
    for drv in (host, dev):
        _program(drv)
        drv.set_species_tree(parent, tau0, thetas)
        drv.set_tau_prior(3.0, 3.0 / tau0[-1])
        drv.set_theta_prior(2.0, 1000.0, 0.001)
        drv.set_finetune(0.003, 0.005, 0.0008, 0.2)
    walk(host, dev, iters, nloci, tol=1e-9)
    _finish(host, dev, tau0, thetas)
    host.close(); dev.close(); eng.close()


def _tips24(n=12):
    """the 24-tip loci of test_gpu_bigsampler.py::test_big_sampler_on_24_tip_loci_with_scalers (its first 12 are these 12)"""
    rng = np.random.default_rng(5)
    parent, tau0, thetas = synth.species_tree_arrays(4, 0.004)
    species = [k // 6 for k in range(24)]
    data = []
    for _ in range(n):
        left, right, times, root = _msc_start_tree(species, parent, tau0, thetas, rng)
        base = "".join(rng.choice(list("ACGT"), 200))
        seqs = ["".join(c if rng.random() > 0.04 else rng.choice(list("ACGT")) for c in base) for _ in range(24)]
        pats, w = bpp_amd.compress_site_patterns(seqs, True, True)
        data.append(dict(seqs=pats, weights=w, left=left, right=right, times=times, root=root, states=4, rate_cats=1, model="jc69", rates=np.ones(1)))
    return data, species, (parent, tau0, thetas)


def test_big_sampler_program_moves_on_24_tip_loci_with_scalers():
    eng = bpp_amd.Engine(0)
    data, species, (parent, tau0, thetas) = _tips24()
    host = hostdrv.hip_driver(eng, tape.make_engine_loci(eng, data, True), data, seed=3, scaling=True)
    dev = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, data, True), data, seed=3)
    for drv in (host, dev):
        _program(drv)
        drv.set_species_tree(parent, tau0, thetas)
        for i in range(len(data)):
            drv.set_tip_species(i, species)
        drv.set_tau_prior(3.0, 3.0 / tau0[-1])
        drv.set_theta_prior(2.0, 500.0, 0.001)
        drv.set_finetune(0.002, 0.003, 0.0004, 0.1)
    walk(host, dev, 2, len(data), tol=1e-9)
    _finish(host, dev, tau0, thetas, taus_moved=False)
    for i in range(len(data)):
        assert [int(x) for x in dev.tree(i)["pop"]] == [int(x) for x in host.tree(i)["pop"]]
    host.close(); dev.close(); eng.close()


def test_big_sampler_program_moves_on_the_frogs_loci():
    gold = json.load(open(os.path.join(G, "input_pipeline.json")))
    recs = seqio.load_dataset(os.path.join(G, "frogs", "frogs.txt"), os.path.join(G, "frogs", "frogs.Imap.txt"), gold["species"], [1, 1, 1, 1], model="jc69")
    eng = bpp_amd.Engine(0)
    parent = [4, 4, 5, 6, 5, 6, -1]                       # K C L H | KC KCL root
    tau0 = [0.0] * 4 + [0.01, 0.02, 0.03]
    thetas = [0.02] * 7
    rng = np.random.default_rng(9)
    data = []
    for r in recs:
        left, right, times, root = _msc_start_tree(r["species"], parent, tau0, thetas, rng)
        data.append(dict(seqs=r["seqs"], weights=r.get("weights", np.ones(len(r["seqs"][0]))), left=left, right=right, times=times, root=root,
                         states=4, rate_cats=1, model="jc69", rates=np.ones(1)))
    assert max(len(r["seqs"]) for r in recs) > 16
    host = hostdrv.hip_driver(eng, [seqio.make_locus(eng, r) for r in recs], data, seed=8)
    dev = bpp_amd.Sampler(eng, [seqio.make_locus(eng, r) for r in recs], data, seed=8)
    for drv in (host, dev):
        _program(drv)
        drv.set_species_tree(parent, tau0, thetas)
        for i, r in enumerate(recs):
            drv.set_tip_species(i, r["species"])
        drv.set_tau_prior(3.0, 100.0)
        drv.set_theta_prior(3.0, 150.0, 0.003)
        drv.set_finetune(0.004, 0.004, 0.002, 0.1)
    walk(host, dev, 2, len(data), tol=1e-9)
    _finish(host, dev, tau0, thetas, taus_moved=False)
    host.close(); dev.close(); eng.close()


def _make24(eng, data, species, stree, kernel, program, theta_prior, finetune=(0.002, 0.003, 0.0004, 0.1), seed=3, slide=0.1):
    parent, tau0, thetas = stree
    smp = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, data, True), data, seed=seed)
    if kernel:
        smp.set_proposal_kernel(1)
    if program:
        smp.set_program_moves(True, slide)
    smp.set_species_tree(parent, tau0, thetas)
    for i in range(len(data)):
        smp.set_tip_species(i, species)
    smp.set_tau_prior(3.0, 3.0 / tau0[-1])
    if theta_prior:
        smp.set_theta_prior(2.0, 500.0, 0.001)
    smp.set_finetune(*finetune)
    smp.initialize()
    assert smp.kind() == "big"
    return smp


def test_what_the_big_tree_sampler_refuses_with_bpp_s_kernel():
    """BPP's proposal kernel comes with the program's moves and a theta prior: anything else fails when the run starts (no
    silent fall-back to the uniform kernel); the full combination runs and moves taus and thetas"""
    eng = bpp_amd.Engine(0)
    data, species, stree = _tips24(4)
    for program, theta_prior in ((False, True), (True, False)):
        smp = _make24(eng, data, species, stree, True, program, theta_prior)
        with pytest.raises(bpp_amd.BpaError, match="program's moves"):
            smp.iterate(1)
        smp.close()
    smp = _make24(eng, data, species, stree, True, True, True)
    smp.iterate(40)            # (a rubber band over four loci's 92 gene nodes is accepted a few times in ten: not in every iteration)
    assert smp.taus() != list(stree[1]) and smp.thetas() != list(stree[2])
    g = smp.gibbs_counters()
    assert g[0] > 0
    smp.close(); eng.close()


def _state(smp, n):
    return smp.taus(), smp.thetas(), [(list(t["left"]), list(t["right"]), list(t["time"]), t["root"], t["lnl"], t["logpr"]) for t in (smp.tree(i) for i in range(n))]


def test_the_step_length_rule_on_the_big_tree_sampler():
    """bpa_sampler_adapt_finetune / bpa_sampler_burnin on a big-tree sampler with the program's moves: the per-locus counts come
    from the trees (BTree::pj_*), tau / mix / theta window from the decisions' state on the device.

    Bars after burnin(400) + 300 iterations from the program's default step lengths: those of
    test_finetune_adaptation.py::test_the_rule_on_the_generic_sampler (0.15-0.45 for gspr, tau, mix; 0.2-0.6 for gage).
    Observed pjumps on one MI355X (12 loci of 24 tips): gage 0.573, gspr 0.262, tau 0.396, mix 0.283
    (theta window 0.322), with the step lengths burnin(400) ended at: gage 99 (the age window is capped by its bounds, as on the
    generic sampler), gspr 0.000399, tau 0.000432, mix 0.0672, theta 0.0156.
    """
    eng = bpp_amd.Engine(0)
    data, species, stree = _tips24()
    n = len(data)
    # below 200 iterations the program resets nothing: burnin(150) is iterate(150)
    a = _make24(eng, data, species, stree, True, True, True)
    b = _make24(eng, data, species, stree, True, True, True)
    ft = a.burnin(150)
    b.iterate(150)
    assert (ft["gage"], ft["gspr"], ft["tau"], ft["mix"], ft["theta"]) == (0.002, 0.003, 0.0004, 0.1, 0.001)
    assert _state(a, n) == _state(b, n)
    b.close()
    # one application of the rule is bpa_finetune_onestep of the acceptance proportion, per move type
    prev = dict(ft)
    pj, ft1 = a.adapt_finetune()
    L = bpp_amd.lib()
    for k in bpp_amd.Sampler.FT_NAMES:
        if pj[k] >= 0:
            assert 0 <= pj[k] <= 1
            assert ft1[k] == L.bpa_finetune_onestep(pj[k], prev[k]), (k, pj[k], prev[k], ft1[k])
        else:
            assert ft1[k] == prev[k], k
    assert all(pj[k] >= 0 for k in ("gage", "gspr", "tau", "mix")), pj
    pj0, ft2 = a.adapt_finetune()                       # nothing proposed since: the step lengths stay
    assert all(v < 0 for v in pj0.values()) and ft2 == ft1
    a.close()
    # the burn-in from the program's defaults (bpp.c:530-549), then the chain accepts what the rule aims at
    c = _make24(eng, data, species, stree, True, True, True, finetune=(5.0, 0.001, 0.001, 0.3))
    ftc = c.burnin(400)
    assert ftc["gage"] != 5.0 and ftc["tau"] != 0.001 and ftc["mix"] != 0.3
    c.iterate(300)
    pjc, _ = c.adapt_finetune()
    print(f"[big-program] pjump after burnin(400) + 300: {pjc}  finetune {ftc}")
    for k in ("gspr", "tau", "mix"):
        assert 0.15 < pjc[k] < 0.45, (k, pjc, ftc)
    assert 0.2 < pjc["gage"] < 0.6, (pjc, ftc)
    c.close()
    # without the program's moves there are no counts by move type to go on: both calls fail, before any iteration runs
    u = _make24(eng, data, species, stree, False, False, True)
    u.iterate(1)
    before = _state(u, n)
    with pytest.raises(bpp_amd.BpaError, match="program's moves"):
        u.adapt_finetune()
    with pytest.raises(bpp_amd.BpaError, match="program's moves"):
        u.burnin(400)
    assert _state(u, n) == before
    u.close(); eng.close()
