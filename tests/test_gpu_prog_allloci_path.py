"""The program-moves instances of the persistent kernel (csrc/sweep2.hpp: iter_kernel<.., true, true[, true]>) with the shorter
path between the barriers of an all-loci step (NOTES §27):

  * a locus's density terms and their sum are refreshed ONCE an iteration, behind MIX; THETA, the TAUs and MIX leave `logpr`
    and the terms alone and form only the statistic T2h (the control wave makes the density change from k_p and the T2h sums);
    the lanes' node sets and counts are made in the first all-loci step only;
  * the iteration's first proposal of the species tree is made by the control wave DURING the sweep and handed to the loci
    waves under the iteration's number.

None of it may show: (a) the trajectory is the C host driver's, (b) it does not depend on where launches end, (c) the `logpr` a
caller reads is the tree's density, (d) the instance whose sets change waves gives the identity instance's bits, and a launch
that gives up is run again from an untouched state, (e) a long run's decision log — with gamma blocks that went through
prog_gammas_redo in it — is the parent commit's, line for line (tests/golden/prog_declog_64x200.txt, recorded on one MI355X
from the parent build, commit e8908df).

The seeds of (a): the host driver and the device part ways where a last-bit difference of log / sqrt (device libm against
glibc) turns a decision or moves an age beyond 1e-10 (NOTES §18, "a finding beside the point"); of the chain seeds 5, 6, 7, ...
the first for which the PARENT build passes the same comparison over the same 40 iterations is taken, per data set: 10 for the
four-taxon set (5 .. 9 part ways with the host driver between iterations 4 and 40 on the parent build too), 7 for the 8-tip set."""
import os
import re

import numpy as np
import pytest

import bpp_amd
from bpp_amd import synth
import hostdrv
import tape
from invariants import msc_recompute, LOGPR_TOL
from common import rel

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prog_declog_64x200.txt")
DENSE, IDENTITY, DECLOG = 4096, 8192, 256


def _setup(drv, taxa, slide=0.3):
    parent, tau0, thetas = synth.species_tree_arrays(taxa)
    drv.set_proposal_kernel(1)
    drv.set_program_moves(True, slide)
    drv.set_species_tree(parent, tau0, thetas)
    drv.set_tau_prior(3.0, 3.0 / tau0[-1])
    drv.set_theta_prior(2.0, 1000.0, 0.0004)
    drv.set_finetune(0.003, 0.004, 0.0004, 0.1)
    drv.initialize()
    return parent


def _device(eng, data, taxa, seed, **options):
    dev = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, data), data, seed=seed, **options)
    _setup(dev, taxa)
    assert dev.kind() == "persistent"
    return dev


def _state(dev, n):
    """everything a getter shows: ages, trees, buffer indices, populations, lnL, logpr; taus, thetas; the counters"""
    s = dev.summary()
    return dict(trees=[dev.tree(i) for i in range(n)], taus=dev.taus(), thetas=dev.thetas(),
                counts=(s["proposals"], s["accepted"]), gibbs=tuple(dev.gibbs_counters()), total=s["total_lnl"])


def _same(a, b, what):
    assert a["taus"] == b["taus"] and a["thetas"] == b["thetas"], what
    assert a["counts"] == b["counts"] and a["gibbs"] == b["gibbs"] and a["total"] == b["total"], what
    for i, (x, y) in enumerate(zip(a["trees"], b["trees"])):
        for key in x:
            assert np.array_equal(x[key], y[key]), (what, i, key, x[key], y[key])


def trajectory_against_host(taxa, nloci, sites, data_seed, seed, chunks):
    """the comparison of tests/test_gpu_prog_decisions.py: after every call the host driver's proposal / acceptance counts and
    Gibbs counters; at the end its taus, thetas (1e-10 relative) and every tree (parents ==, ages 1e-10 relative)"""
    eng = bpp_amd.Engine(0)
    try:
        data = synth.make_dataset(nloci, sites, taxa, "jc69", 1, seed=data_seed)
        host = hostdrv.hip_driver(eng, tape.make_engine_loci(eng, data), data, seed=seed)
        _setup(host, taxa)
        dev = _device(eng, data, taxa, seed)
        for chunk in chunks:
            for _ in range(chunk):
                host.iterate()
            dev.iterate(chunk)
            s = dev.summary(); hp, ha, _ = host.counters()
            assert (s["proposals"], s["accepted"]) == (hp, ha), chunk
            assert dev.gibbs_counters() == host.gibbs_counters(), chunk
        assert np.allclose(dev.taus(), host.taus(), rtol=1e-10, atol=0) and np.allclose(dev.thetas(), host.thetas(), rtol=1e-10, atol=0)
        for i in range(nloci):
            a, b = dev.tree(i), host.tree(i)
            assert [int(x) for x in a["parent"]] == [int(x) for x in b["parent"]] and np.allclose(a["time"], b["time"], rtol=1e-10, atol=0), i
        host.close(); dev.close()
    finally:
        eng.close()


# (taxa, loci, sites, data seed, chain seed): 200 four-taxon loci of 60 sites = iter_kernel<4, true, true> on several workgroups;
# one 8-tip set of 64 loci = iter_kernel<8, true, true>.  The chain seeds: see the module's docstring
TRAJ = [(4, 200, 60, 2700, 10), (8, 64, 60, 2708, 7)]
TRAJ_CHUNKS = (1, 1, 1, 37)          # 40 iterations: launches of one iteration, then one launch of many


@pytest.mark.parametrize("taxa,nloci,sites,data_seed,seed", TRAJ, ids=[f"{t[0]}x{t[1]}" for t in TRAJ])
def test_a_trajectory_is_the_host_drivers(taxa, nloci, sites, data_seed, seed):
    trajectory_against_host(taxa, nloci, sites, data_seed, seed, TRAJ_CHUNKS)


# ---- (b), (c): one run in three ways of cutting it into launches
SPLIT_SETS = {"4x200": (4, 200, 60, 2700, {}), "handover-40": (4, 40, 300, 140, dict(debug=DENSE))}
_split_runs = {}


def _split(name):
    """24 iterations (+ 3: whatever the getters do not show — the loci's streams, the global stream — shows in what follows) as
    one launch, as launches of one iteration, and with a sample trace at every = 3, whose launches end at the rows"""
    if name not in _split_runs:
        taxa, nloci, sites, data_seed, options = SPLIT_SETS[name]
        eng = bpp_amd.Engine(0)
        data = synth.make_dataset(nloci, sites, taxa, "jc69", 1, seed=data_seed)
        out = {}
        for how in ("one", "singles", "traced"):
            dev = _device(eng, data, taxa, 11, **options)
            if how == "traced":
                dev.set_trace(3)
            if how == "singles":
                for _ in range(24):
                    dev.iterate(1)
            else:
                dev.iterate(24)
            first = _state(dev, nloci)
            dev.iterate(3)
            out[how] = (first, _state(dev, nloci))
            if how == "traced":
                assert list(dev.trace()["iteration"]) == list(range(3, 28, 3))
            dev.close()
        eng.close()
        _split_runs[name] = (data, synth.species_tree_arrays(taxa)[0], out)
    return _split_runs[name]


@pytest.mark.parametrize("name", sorted(SPLIT_SETS))
def test_b_where_launches_end_does_not_show(name):
    """a refresh missing at a launch's end, a first proposal drawn twice or not at all would show here"""
    _, _, out = _split(name)
    for how in ("singles", "traced"):
        for k, when in enumerate(("after 24", "after 27")):
            _same(out["one"][k], out[how][k], (name, how, when))
    assert out["one"][0]["taus"] != out["one"][1]["taus"] and out["one"][0]["counts"][1] > 0          # (the chain moves)


@pytest.mark.parametrize("name", sorted(SPLIT_SETS))
def test_c_logpr_is_the_trees_density(name):
    """every locus's downloaded logpr against the CPU recompute of tests/invariants.py from the downloaded tree, taus and thetas"""
    data, sparent, out = _split(name)
    for how, (st, _) in sorted(out.items()):
        worst = 0.0
        for i, t in enumerate(st["trees"]):
            tips = len(data[i]["seqs"])
            pop, want = msc_recompute(t, tips, sparent, st["taus"], st["thetas"], list(range(tips)))
            assert pop == [int(x) for x in t["pop"]], (how, i)
            e = rel(t["logpr"], want)
            worst = max(worst, e)
            assert e < LOGPR_TOL, (how, i, t["logpr"], want, e)
        print(f"[allloci-path] {name} {how}: logpr within {worst:.2e} of the recompute over {len(st['trees'])} loci")


# ---- (d): the instance whose sets change waves
def test_d_handover_instance_gives_the_identity_instances_bits(capfd):
    """33 loci dealt densely: five waves of loci in one workgroup, the fifth set of one locus (the smallest set of
    tests/test_gpu_sweep_handover.py) — iter_kernel<4, true, true, true>; 30 iterations as launches of 1, 1, 1, 7 and 20"""
    eng = bpp_amd.Engine(0)
    data = synth.make_dataset(33, 300, 4, "jc69", 1, seed=133)
    chunks = (1, 1, 1, 7, 20)
    got = {}
    for what, dbg in (("handover", DENSE | 16), ("identity", DENSE | IDENTITY | 16)):
        dev = _device(eng, data, 4, 5, debug=dbg)
        for c in chunks:
            dev.iterate(c)
        got[what] = _state(dev, 33)
        dev.close()
        err = capfd.readouterr().err
        assert ("sets change waves: yes" in err) == (what == "handover"), err[-1500:]
    _same(got["handover"], got["identity"], "hand-over against identity")
    eng.close()


def test_d_a_launch_that_gives_up_is_run_again_from_an_untouched_state():
    """the give-up switch (debug bit 1024, set for the second launch by the option inject = 2): every workgroup gives up at the
    launch's first wait, the launch stores nothing and its 10 iterations — first proposals made during the sweeps among them —
    run again: the state a run without it reaches, to the bit"""
    eng = bpp_amd.Engine(0)
    data = synth.make_dataset(40, 300, 4, "jc69", 1, seed=140)
    got = {}
    for what, options in (("inject", dict(debug=DENSE, inject=2)), ("plain", dict(debug=DENSE))):
        dev = _device(eng, data, 4, 5, **options)
        for c in (10, 10, 10):
            dev.iterate(c)
        got[what] = _state(dev, 40)
        dev.close()
    _same(got["inject"], got["plain"], "a launch given up and run again")
    eng.close()


# ---- (e): a long run's decision log
DECLOG_LOCI, DECLOG_DATA_SEED, DECLOG_SEED, DECLOG_LAUNCHES = 64, 164, 7, (100, 100)      # 7 decisions an iteration: a launch's log holds 1 000


def decision_log(capfd):
    """200 iterations of 64 four-taxon loci as two launches with the decision log on: the log's lines — step, ln of the acceptance
    ratio to 17 digits, the decision.  A launch's log is printed when the state is next downloaded"""
    eng = bpp_amd.Engine(0)
    data = synth.make_dataset(DECLOG_LOCI, 300, 4, "jc69", 1, seed=DECLOG_DATA_SEED)
    dev = _device(eng, data, 4, DECLOG_SEED, debug=DECLOG)
    capfd.readouterr()
    lines = []
    for n in DECLOG_LAUNCHES:
        dev.iterate(n)
        dev.summary(); dev.tree(0)
        err = capfd.readouterr().err
        got = [ln for ln in err.splitlines() if re.match(r"\[smp2\] (theta|tau|mix) ", ln)]
        assert len(got) == 7 * n, (len(got), err[-800:])
        lines += got
    dev.close(); eng.close()
    return lines


def test_e_decision_log_with_redone_gamma_blocks_is_the_parents(capfd):
    """A gamma block goes back through prog_gammas_redo when a variate fails Marsaglia-Tsang's test at the first round: about one
    block in a hundred (sweep2.hpp: draw_gammas), 4 blocks an iteration, so about eight of this run's 800 — the chance of none
    is 0.99^800 = 3e-4; the log itself does not mark them.  Behind a redone block the stream stands elsewhere than the block's scan
    left it, and the next proposal — the iteration's first among them, now drawn during the sweep — starts from there.  1 400
    decisions, every ln of an acceptance ratio to its last digit: the parent build's"""
    want = [ln.rstrip("\n") for ln in open(GOLDEN)]
    got = decision_log(capfd)
    assert len(want) == len(got) == 1400
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, (k, a, b)
