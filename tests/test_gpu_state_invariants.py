"""Every kind of device sampler after a LONG run: what it holds per locus — tree, buffer indices, population labels, MSC
density, log-likelihood — and what its loci's device buffers hold (root term, every P-matrix, every inner CLV, scale counters)
against a from-scratch recompute on the CPU (tests/invariants.py: check_state; the oracle and a one-locus prior driver), for
EVERY locus, at growing iteration counts.  No host driver runs alongside: after ~25 iterations the two trajectories split on a
last-bit log / sqrt — the invariants do not need them to agree.  A chunk longer than 1 is the multi-iteration launch
of the persistent kernel, the path bench.py times.  CPU twin, with the checker's own failure cases: tests/test_state_invariants.py.

Measured on one MI355X (largest difference from the ORACLE's recompute over all loci and checkpoints of a case; `acc` = accepted /
proposals at the end; P-matrices: largest ulp distance among the matrices within 8 ulp, and the largest absolute difference among
those that pass by the 5e-16 absolute bar instead; logpr was 0.0 in every case, inner CLVs and scale counters are compared with ==):

  case                          iterations  loci   acc   lnl       root buffer  total     P ulps  P abs
  headline (persistent)               3000  2000  0.43   3.0e-16   3.0e-16      0.0       0       1.1e-16
  8 tips, BPP's kernel                1000   600  0.47   2.8e-16   2.8e-16      0.0       0       1.1e-16
  6 tips, uniform windows             1000   600  0.40   3.9e-16   3.9e-16      0.0       0       1.1e-16
  lane-group edges 4 / 8 tips          500  1-65  .23-.38  2.4e-16 2.4e-16      0.0       0       1.1e-16
  several sequences per species       1000   120  0.88   4.8e-16   4.8e-16      0.0       3       1.1e-16
    ... with the program's moves      1000   120  0.84   2.3e-16   2.3e-16      0.0       5       1.1e-16
  one launch per step (sweep)          200   300  0.50   0.0       0.0          0.0       0       1.1e-16
  generic, GTR+G4 + parameter moves    300    60  0.34   2.3e-16   2.3e-16      0.0       8       1.1e-16
    ... 700 loci, part-batches          60   700  0.34   2.5e-16   2.5e-16      0.0       8       1.1e-16
  generic forced on JC69, chain 0 / 1  200    40  0.53   0.0       0.0          0.0       0       0.0
  generic, LG+G4                       100    40  0.60   1.9e-16   1.9e-16      0.0       8       2.2e-16
    ... 300 loci, two streams           40   300  0.65   1.9e-16   1.9e-16      0.0       8       2.2e-16
  generic, anopheles                   200   100  0.40   3.6e-16   3.6e-16      0.0       0       1.1e-16
  big, 24 tips with scalers             50    12  0.49   2.9e-16   2.9e-16      0.0       0       1.1e-16
  big, frogs (diploid)                  30     5  0.44   0.0       0.0          0.0       0       0.0
  composite                            100   133  0.60   1.1e-16   1.1e-16      2.0e-16   4       1.1e-16
  at the samplers' pattern- and tip-count limits (tests/test_gpu_sampler_limits.py, loci of exact shape; uniform / program's moves):
  persistent, 4-tip form, 1-64 patterns 200    40  0.69   1.7e-16   1.7e-16      0.0       6       1.1e-16
  persistent, 8-tip form, 1-64 patterns 200    23  .59-.64  2.1e-16 2.1e-16      0.0       6       1.1e-16
  persistent, 2-8 tips in one sampler  200    24  .65-.77  3.5e-16 3.5e-16      0.0       3       1.1e-16
  generic, 4 tips, one 65-pattern locus 200    40  .69-.71  1.5e-16 1.5e-16      0.0       6       1.1e-16
  composite, 64 / 65 patterns + GTR+G4 200   134  0.53   5.5e-16   5.5e-16      6.4e-16   6       1.1e-16
  generic, 16 tips, JC69 1-255 patterns 200     4  .52-.57  2.0e-16 2.0e-16      0.0       5       1.1e-16
    ... GTR+G4, 252 lanes, param. moves 200     5  .26-.57  1.4e-16 1.4e-16      0.0       8       4.4e-16
    ... GTR, 3 categories, 255 lanes   200     5  .55-.57  1.3e-16 1.3e-16      0.0       8       0.0
    ... GTR, 8 categories, 248 lanes   200     5  .55-.63  1.8e-16 1.8e-16      0.0       5       0.0
    ... 12 and 16 tips side by side    200     6  .55-.60  0.0       0.0          0.0       3       0.0
  big, 17 tips, 30 / 300 patterns       30     3  .30-.50  0.0       0.0          0.0       0       0.0
  big, 64 tips, 30 / 300 patterns       30     3  .25-.47  0.0       0.0          0.0       0       1.1e-16
  where the scale counters fire (tests/test_gpu_scaling_fires.py on the sets of tests/firing.py, big-tree sampler with scale buffers,
  uniform / program's moves; `nodes`: inner nodes with a non-zero counter in the ORACLE's recompute, per locus, after the first
  iteration -> after the last; `top`: the largest counter at the start tree -> after the last):
  case                          iterations  loci   acc   lnl       root buffer  total     P ulps  P abs    nodes                top
  big, 17 + 24 tips, f = 1e-6           30   3+3  .31-.38  0.0     0.0          0.0       0       0.0      2-6 -> 1-7           2 -> 1
  big, 24 tips, f = 1e-6                30     6  .29-.37  0.0     0.0          0.0       0       0.0      2-6 -> 1-7           2 -> 1
  big, 24 tips, GTR+G4, f = 1e-6        30     6  .30-.37  0.0     0.0          0.0       0       0.0      2-5 -> 1-4           2 -> 1
  big, 64 tips, f = 1e-3                30     3  .28-.34  0.0     0.0          0.0       0       0.0      4-6 -> 3-6           3 -> 2-3
  (at branch lengths of 1e-10 .. 1e-8 expm1(x) is x on both sides: every P-matrix, and with it every lnL, had the oracle's bits; the
  batched plans, the tapes — 220 steps per locus, JC69 and GTR+G4 — and the host driver's 5 iterations of that file were 0.0 from the
  oracle / the reference as well)
  (generic: chain=0 and 1 gave the same figures; big: with and without scale buffers gave the same figures.  On the loci of
  tests/shapes.py no scale counter of the oracle's recompute is non-zero at 17 or 64 tips — those cases compare zeros; the counters
  that are non-zero are the four cases above and the golden loci 9-11 / K1 vectors of tests/test_gpu_parity.py)

No invariant failed on the device.  Reads between iterations (the last test): on the library before the marks of
gs_mark_roots, all 180 reads (60 loci x single-locus call / plan / batch) of the buffer the tree then named as the root's returned
-inf without an error — the root's buffer had never been written; with the marks all 180 are refused with a message naming the remedy.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import bpp_amd
from bpp_amd import synth, seqio, api
import tape
from common import rel
from invariants import check_state, several_sequences_data, moved, oracle_locus, LNL_TOL_SUBST

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WORST = {}               # case -> largest differences seen (printed per case: pytest -s / -rP shows them)


def grow(case, dev, chunks, tau0, thetas0, **kw):
    """iterate to each cumulative count of `chunks`, the whole state checked after each; then: the chain moved"""
    done = 0
    worst = WORST.setdefault(case, {})
    for upto in chunks:
        dev.iterate(upto - done)
        done = upto
        check_state(dev, worst=worst, **kw)
    s = dev.summary()
    moved(dev, tau0, thetas0, s["proposals"], s["accepted"])
    print(f"[invariants] {case}: {done} iterations, {len(kw['data'])} loci, accepted {s['accepted'] / s['proposals']:.2f}: "
          + ", ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items())))


def make(eng, data, stree, seed, moves, species=None, prior=(2.0, 1000.0, 0.0004), finetune=(0.003, 0.004, 0.0004, 0.1), tau_prior=None,
         loci=None, slide=0.3, **options):
    """moves: 'uniform' (the library's own windows), 'bpp' (BPP's kernel), 'program' (BPP's kernel and the program's moves)"""
    parent, tau0, thetas = stree
    loci = tape.make_engine_loci(eng, data) if loci is None else loci
    dev = bpp_amd.Sampler(eng, loci, data, seed=seed, **options)
    if moves != "uniform":
        dev.set_proposal_kernel(1)
    if moves == "program":
        dev.set_program_moves(True, slide)
    dev.set_species_tree(parent, tau0, thetas)
    if species is not None:
        for i in range(len(data)):
            dev.set_tip_species(i, species[i])
    dev.set_tau_prior(*(tau_prior or (3.0, 3.0 / tau0[-1])))
    dev.set_theta_prior(*prior)
    dev.set_finetune(*finetune)
    return dev, loci


def test_headline_shape():
    """bench.py's flagship shape on the persistent kernel, BPP's kernel with the program's moves; the last chunk is ONE launch
    of 2 000 iterations"""
    eng = bpp_amd.Engine(0)
    data = synth.make_dataset(2000, 1000, 4, "jc69", 1, seed=3)
    stree = synth.species_tree_arrays(4)
    dev, loci = make(eng, data, stree, 5, "program", prior=(2.0, 1000.0, 0.0003), finetune=(0.0012, 0.0015, 0.0002, 0.05))
    dev.initialize()
    assert dev.kind() == "persistent"
    grow("headline", dev, (1, 10, 100, 1000, 3000), stree[1], stree[2], data=data, species_parent=stree[0], loci=loci)
    dev.close(); eng.close()


@pytest.mark.parametrize("taxa,moves", [(8, "bpp"), (6, "uniform")])
def test_persistent_kernel_eight_tip_form(taxa, moves):
    eng = bpp_amd.Engine(0)
    data = synth.make_dataset(600, 500, taxa, "jc69", 1, seed=7)
    stree = synth.species_tree_arrays(taxa)
    dev, loci = make(eng, data, stree, 11, moves, prior=(2.0, 1000.0, 0.0003) if taxa == 8 else (2.0, 100.0, 0.002),
                     finetune=(0.0012, 0.0015, 0.0002, 0.05) if taxa == 8 else (0.01, 0.012, 0.002, 0.05))
    dev.initialize()
    assert dev.kind() == "persistent"
    grow(f"persistent-{taxa}-{moves}", dev, (1, 10, 100, 1000), stree[1], stree[2], data=data, species_parent=stree[0], loci=loci)
    dev.close(); eng.close()


@pytest.mark.parametrize("taxa", [4, 8])
@pytest.mark.parametrize("nloci", [1, 13, 65])
def test_persistent_kernel_at_lane_group_edges(taxa, nloci):
    """one lane group, one partial wave, one locus beyond a workgroup"""
    eng = bpp_amd.Engine(0)
    data = synth.make_dataset(nloci, 300, taxa, "jc69", 1, seed=100 + nloci)
    stree = synth.species_tree_arrays(taxa)
    dev, loci = make(eng, data, stree, 5, "program")
    dev.initialize()
    assert dev.kind() == "persistent"
    grow(f"edges-{taxa}-{nloci}", dev, (7, 500), stree[1], stree[2], data=data, species_parent=stree[0], loci=loci)
    dev.close(); eng.close()


@pytest.mark.parametrize("program", [False, True])
def test_several_sequences_per_species(program):
    """tip populations hold coalescences, gene nodes cross the species boundary both ways, the tip populations' thetas move"""
    eng = bpp_amd.Engine(0)
    data, species, stree = several_sequences_data()
    dev, loci = make(eng, data, stree, 4, "program" if program else "uniform", species=[species] * len(data), slide=0.5,
                     tau_prior=(3.0, 1000.0), prior=(2.0, 700.0, 0.002), finetune=(0.003, 0.004, 0.0008, 0.2))
    dev.initialize()
    assert dev.kind() == "persistent"
    grow(f"several-{int(program)}", dev, (8, 1000), stree[1], stree[2], data=data, species_parent=stree[0], loci=loci,
         tip_species=[species] * len(data))
    assert sum(sum(int(x) == 2 for x in dev.tree(i)["pop"][6:]) != 1 for i in range(len(data))) > 0
    dev.close(); eng.close()


def test_one_launch_per_step():
    eng = bpp_amd.Engine(0)
    data = synth.make_dataset(300, 400, 4, "jc69", 1, seed=17)
    stree = synth.species_tree_arrays(4)
    dev, loci = make(eng, data, stree, 23, "uniform", prior=(2.0, 1000.0, 0.001), finetune=(0.003, 0.005, 0.0008, 0.2), implementation="sweep")
    dev.initialize()
    assert dev.kind() == "sweep"
    grow("sweep", dev, (5, 200), stree[1], stree[2], data=data, species_parent=stree[0], loci=loci)
    dev.close(); eng.close()


def _gtr_sampler(eng, nloci, seed=41):
    data = synth.make_dataset(nloci, 300, 8, "gtr", 4, seed=seed)
    stree = synth.species_tree_arrays(8)
    dev, loci = make(eng, data, stree, 43, "program", finetune=(0.003, 0.005, 0.0004, 0.05))
    dev.set_subst_moves(0.3, 0.4, 0.8, 1.0, 1.0)
    for i, d in enumerate(data):
        dev.set_subst_model(i, d["freqs"], d["exch"], 0.5)
    return data, stree, dev, loci


@pytest.mark.parametrize("nloci,chunks", [(60, (3, 30, 300)), (700, (2, 60))])
def test_generic_sampler_gtr_gamma_with_parameter_moves(nloci, chunks):
    """BASELINE config 3's kind: GTR + Gamma4, the program's moves and the per-locus frequency / exchangeability / alpha moves; the
    oracle takes each locus's CURRENT parameters.  700 loci: the per-locus steps as part-batches on several streams"""
    eng = bpp_amd.Engine(0)
    data, stree, dev, loci = _gtr_sampler(eng, nloci)
    dev.initialize()
    assert dev.kind() == "generic"
    assert (dev.streams() > 1) == (nloci >= 700)
    grow(f"gtr-{nloci}", dev, chunks, stree[1], stree[2], data=data, species_parent=stree[0], loci=loci, subst=True)
    assert any(dev.get_subst_model(i)[2] != 0.5 for i in range(nloci))
    dev.close(); eng.close()


@pytest.mark.parametrize("chain", [0, 1])
def test_generic_sampler_forced_on_jc69_loci(chain):
    """the per-locus steps as a launch each (chain=0) and as ONE launch (1)"""
    eng = bpp_amd.Engine(0)
    data = synth.make_dataset(40, 300, 8, "jc69", 1, seed=19)
    stree = synth.species_tree_arrays(8)
    dev, loci = make(eng, data, stree, 29, "uniform", prior=(2.0, 1000.0, 0.001), finetune=(0.003, 0.005, 0.0008, 0.2),
                     implementation="generic", chain=chain)
    dev.initialize()
    assert dev.kind() == "generic"
    grow(f"generic-jc-chain{chain}", dev, (3, 200), stree[1], stree[2], data=data, species_parent=stree[0], loci=loci)
    dev.close(); eng.close()


@pytest.mark.parametrize("nloci,chunks", [(40, (3, 100)), (300, (2, 40))])
def test_generic_sampler_amino_acid_loci(nloci, chunks):
    """BASELINE config 4's kind: LG + Gamma4 (20 states), the program's moves; 300 loci: two streams"""
    eng = bpp_amd.Engine(0)
    data = synth.make_dataset(nloci, 300, 6, "lg", 4, seed=41)
    stree = synth.species_tree_arrays(6)
    dev, loci = make(eng, data, stree, 43, "program", finetune=(0.003, 0.005, 0.0004, 0.05))
    dev.initialize()
    assert dev.kind() == "generic"
    assert (dev.streams() == 2) == (nloci >= 128)
    grow(f"lg-{nloci}", dev, chunks, stree[1], stree[2], data=data, species_parent=stree[0], loci=loci)
    dev.close(); eng.close()


def test_generic_sampler_on_the_anopheles_data():
    """BASELINE config 5's data, set up as tests/test_gpu_gsampler.py::test_generic_sampler_on_the_anopheles_data (12 tips, 6
    species with two sequences each), with BPP's kernel and the program's moves"""
    species = ["G", "C", "R", "L", "A", "Q"]
    recs = seqio.load_dataset(os.path.join(G, "anopheles", "loci_realign.txt"), os.path.join(G, "anopheles", "Imap.txt"),
                              species, None, model="jc69", cleandata=True)
    parent = [6, 6, 10, 8, 7, 7, 9, 8, 9, 10, -1]
    tau0 = [0.0] * 6 + [0.004, 0.004, 0.008, 0.012, 0.016]
    thetas = [0.02] * 11
    rng = np.random.default_rng(77)
    data = []
    for r in recs:
        left, right, times, root = synth.msc_start_tree(r["species"], parent, tau0, thetas, rng)
        data.append(dict(seqs=r["seqs"], weights=r["weights"], left=left, right=right, times=times, root=root, states=4,
                         rate_cats=1, model="jc69", rates=np.ones(1)))
    sp = [r["species"] for r in recs]
    eng = bpp_amd.Engine(0)
    dev, loci = make(eng, data, (parent, tau0, thetas), 21, "program", species=sp, tau_prior=(2.0, 10.0), prior=(2.0, 100.0, 0.002),
                     finetune=(0.003, 0.003, 0.00002, 0.9))
    dev.initialize()
    assert dev.kind() == "generic"
    grow("anopheles", dev, (5, 200), tau0, thetas, data=data, species_parent=parent, loci=loci, tip_species=sp)
    dev.close(); eng.close()


def test_big_sampler_on_24_tip_loci_with_scalers():
    """the data of tests/test_gpu_bigsampler.py::test_big_sampler_on_24_tip_loci_with_scalers; scale counters compared too"""
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
    dev, loci = make(eng, data, stree, 3, "uniform", species=sp, prior=(2.0, 500.0, 0.001), finetune=(0.002, 0.003, 0.0004, 0.1),
                     loci=tape.make_engine_loci(eng, data, True))
    dev.initialize()
    assert dev.kind() == "big"
    grow("big-scalers", dev, (2, 50), tau0, thetas, data=data, species_parent=parent, loci=loci, tip_species=sp, scaling=True)
    dev.close(); eng.close()


def test_big_sampler_on_the_frogs_loci():
    """BASELINE config 1's data (unphased diploids, 42-60 tips after phasing), set up as
    tests/test_gpu_bigsampler.py::test_big_sampler_on_the_frogs_loci; the root term with the oracle's phase averaging"""
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
    dev, loci = make(eng, data, (parent, tau0, thetas), 8, "uniform", species=sp, tau_prior=(3.0, 100.0), prior=(3.0, 150.0, 0.003),
                     finetune=(0.004, 0.004, 0.002, 0.1), loci=[seqio.make_locus(eng, r) for r in recs])
    dev.initialize()
    assert dev.kind() == "big"
    grow("frogs", dev, (2, 30), tau0, thetas, data=data, species_parent=parent, loci=loci, tip_species=sp)
    dev.close(); eng.close()


def test_loci_of_several_kinds_in_one_sampler():
    """the data of tests/test_gpu_gsampler.py::test_loci_of_several_kinds_in_one_sampler: a part per kind, stepped together"""
    eng = bpp_amd.Engine(0)
    fit = synth.make_dataset(96, 300, 8, "jc69", 1, seed=5)
    wide = synth.make_dataset(7, 8000, 8, "jc69", 1, seed=6, divergence=20.0)
    gtr = synth.make_dataset(30, 300, 8, "gtr", 4, seed=7)
    data = []
    for i in range(96):
        data.append(fit[i])
        if i % 14 == 0: data.append(wide[i // 14])
        if i % 3 == 0 and i // 3 < 30: data.append(gtr[i // 3])
    stree = synth.species_tree_arrays(8)
    dev, loci = make(eng, data, stree, 31, "uniform", prior=(2.0, 1000.0, 0.001), finetune=(0.003, 0.005, 0.0008, 0.2))
    assert dev.kind() == "composite"
    dev.initialize()
    grow("composite", dev, (6, 100), stree[1], stree[2], data=data, species_parent=stree[0], loci=loci)
    dev.close(); eng.close()


READS = ("single-locus", "plan", "batch")


def _root_reads(eng, loci, idx):
    """the root term of every locus on buffer idx[i], read three ways (bpa_locus_root_loglikelihood, one plan over all loci
    with empty update lists, bpa_batch_evaluate); each -> per locus a value or the error's text"""
    n = len(loci)
    single = []
    for i, loc in enumerate(loci):
        try:
            single.append(loc.root_loglikelihood(int(idx[i]), -1))
        except bpp_amd.BpaError as ex:
            single.append(str(ex))
    zeros = np.zeros(n + 1, dtype=np.uint32)
    none_u, none_d, none_op = np.zeros(0, dtype=np.uint32), np.zeros(0), np.zeros(0, dtype=bpp_amd.OP_DTYPE)
    rc, rs = np.array(idx, dtype=np.uint32), np.full(n, -1, dtype=np.int32)
    try:
        p = bpp_amd.Plan(eng, list(loci), zeros, none_u, none_d, zeros, none_op, rc, rs)
        try:
            p.launch()
            plan = list(p.lnl())
        finally:
            p.close()
    except bpp_amd.BpaError as ex:
        plan = [str(ex)] * n
    arr = (C.c_void_p * n)(*[l.h for l in loci])
    b = api.Batch(n, arr, api._up(zeros), api._up(none_u), api._dp(none_d), api._up(zeros), none_op.ctypes.data_as(C.POINTER(api.Op)),
                  api._up(rc), rs.ctypes.data_as(C.POINTER(C.c_int)))
    out = np.zeros(n)
    batch = list(out) if api.lib().bpa_batch_evaluate(eng.h, C.byref(b), api._dp(out)) else [api._err()] * n
    return single, plan, batch


def test_reads_between_iterations_never_return_a_stale_root():
    """The generic sampler's steps do not store the root's CLV (flags bit 11, csrc/gsampler_host.hpp: gs_skip_root_flag); the
    buffers are brought level by a download.  A caller that reads a sampler's locus between iterate calls — single-locus API,
    a plan, bpa_batch_evaluate — and before any getter must get the current value or an ERROR, never a stale number."""
    eng = bpp_amd.Engine(0)
    nloci = 60
    data, stree, dev, loci = _gtr_sampler(eng, nloci)
    dev.initialize()
    dev.iterate(5)                                   # no getter from here on, until the reads are recorded
    tips, inner = 8, 7
    # the root is node 2 tips - 2 of these trees; a node's buffer is k or k + inner (the reference's toggle, locus.c:24-26;
    # gs_upload takes the trees' own indices, which start as clv[k] = k)
    cand = (2 * tips - 2, 2 * tips - 2 + inner)
    reads = {c: _root_reads(eng, loci, [c] * nloci) for c in cand}
    stale, errors = [], 0
    for i in range(nloci):
        t = dev.tree(i)                              # (the first getter: downloads, which levels the buffers)
        c = int(t["clv"][t["root"]])
        assert t["root"] == 2 * tips - 2 and c in cand, (i, t["root"], c)
        full = oracle_locus(data[i], None, None, False, dev.get_subst_model(i)).full_lnl(list(t["left"]), list(t["right"]), list(t["time"]), t["root"])
        assert rel(t["lnl"], full) < LNL_TOL_SUBST, i
        for how, got in zip(READS, reads[c]):
            if isinstance(got[i], str):
                errors += 1
                assert "getter" in got[i] or "download" in got[i], (how, i, got[i])
            elif not rel(got[i], full) < LNL_TOL_SUBST:
                stale.append((how, i, got[i], full))
    print(f"[invariants] reads between iterations: {errors} refused, {len(stale)} stale of {3 * nloci}")
    assert not stale, f"{len(stale)} stale root terms read without an error, e.g. {stale[:3]}"
    # after the getter the same reads are level
    for how, got in zip(READS, _root_reads(eng, loci, [int(dev.tree(i)["clv"][dev.tree(i)["root"]]) for i in range(nloci)])):
        for i in range(nloci):
            assert not isinstance(got[i], str) and rel(got[i], dev.tree(i)["lnl"]) < LNL_TOL_SUBST, (how, i, got[i])
    dev.iterate(2)                                   # and the chain goes on
    check_state(dev, data, stree[0], loci=loci, subst=True)
    dev.close(); eng.close()
