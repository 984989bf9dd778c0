"""Sets of loci that change waves inside the persistent kernel's sweep (csrc/sweep2.hpp: park / pick_up / hand_over; the
schedule: bpa_sweep_schedule).  A workgroup with five waves of loci has two of them on one SIMD; the younger one runs one
step of its own set and one of each set of the three waves that have a SIMD to themselves, and finishes the last of them; each
of the three finishes the set the younger wave held before.  Who holds a set must not show in any result: the device against the C host driver on the same seed, and the device against itself on the identity schedule.

the sampler's debug bits: 4096 deals densely (as few workgroups as hold the waves, so a few dozen loci run as five, six or seven
waves in one workgroup), 8192 keeps the identity schedule, 16 prints workgroup 0's counters — among them whether its sets
changed waves.

Loci (eight to a wave: 300 sites of four taxa are <= 6 patterns a locus): 33 = five sets, the fifth of one locus; 40 = five full
sets; 41 and 56 = six and seven sets (identity schedule); 80 = two workgroups of five, the second's sets counted from 5."""
import importlib.util
import os

import numpy as np
import pytest

import bpp_amd
from bpp_amd import synth
import hostdrv
import tape

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENSE, IDENTITY, COUNTERS = 4096, 8192, 16
CHUNKS = (1, 1, 1, 7)          # a set's holder carries over from launch to launch through HBM only


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _setup(drv, taxa, program=True, bpp=True):
    parent, tau0, thetas = synth.species_tree_arrays(taxa)
    if bpp:
        drv.set_proposal_kernel(1)
    if program:
        drv.set_program_moves(True, 0.3)
    drv.set_species_tree(parent, tau0, thetas)
    drv.set_tau_prior(3.0, 3.0 / tau0[-1])
    drv.set_theta_prior(2.0, 1000.0, 0.0004)
    drv.set_finetune(0.003, 0.004, 0.0004, 0.1)
    drv.initialize()


def _device(eng, data, taxa, dbg, options={}, **kw):
    dev = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, data), data, seed=5, debug=dbg, **options)
    _setup(dev, taxa, **kw)
    assert dev.kind() == "persistent"
    return dev


def _against_host(dev, host, nloci, gibbs=True):
    for chunk in CHUNKS:
        for _ in range(chunk):
            host.iterate()
        dev.iterate(chunk)
        s = dev.summary(); hp, ha, _ = host.counters()
        assert (s["proposals"], s["accepted"]) == (hp, ha), chunk
        if gibbs:
            assert dev.gibbs_counters() == host.gibbs_counters(), chunk
    assert np.allclose(dev.taus(), host.taus(), rtol=1e-10, atol=0) and np.allclose(dev.thetas(), host.thetas(), rtol=1e-10, atol=0)
    for i in range(nloci):
        a, b = dev.tree(i), host.tree(i)
        assert [int(x) for x in a["parent"]] == [int(x) for x in b["parent"]] and np.allclose(a["time"], b["time"], rtol=1e-10, atol=0), i


def _dump(dev, nloci, path):
    rec = _bench().dump_sampler_outputs(dev, nloci, str(path))
    return {f: np.load(os.path.join(str(path), f + ".npy")) for f in rec["files"]}


@pytest.mark.parametrize("nloci", [33, 40, 41, 56, 80])
def test_sets_change_waves_and_nothing_shows(nloci, tmp_path, capfd):
    """BPP's kernel and the program's moves, 10 iterations as launches of 1, 1, 1 and 7: after every call the host driver's
    counts and Gibbs counters, at the end its taus, thetas and every tree; and every array a caller receives equal, to the
    bit, to a device run on the identity schedule"""
    eng = bpp_amd.Engine(0)
    data = synth.make_dataset(nloci, 300, 4, "jc69", 1, seed=100 + nloci)
    host = hostdrv.hip_driver(eng, tape.make_engine_loci(eng, data), data, seed=5)
    _setup(host, 4)
    dev = _device(eng, data, 4, DENSE | COUNTERS)
    _against_host(dev, host, nloci)
    err = capfd.readouterr().err
    five = nloci in (33, 40, 80)
    assert ("sets change waves: yes" in err) == five, err[-2000:]
    if five:
        # workgroup 0: five waves of loci with a role each, marked as changing sets
        line = [ln for ln in err.splitlines() if "SIMD:role of the waves:" in ln][-1]
        assert line.count("*") == 5, line
    got = _dump(dev, nloci, tmp_path / "handover")
    dev.close()
    ref = _device(eng, data, 4, DENSE | IDENTITY)
    for chunk in CHUNKS:
        ref.iterate(chunk)
    want = _dump(ref, nloci, tmp_path / "identity")
    assert sorted(got) == sorted(want) and len(got) >= 11
    for k in want:
        assert got[k].shape == want[k].shape and (got[k] == want[k]).all(), k
    host.close(); ref.close(); eng.close()


def test_uniform_windows_keep_the_identity_schedule(capfd):
    """iter_kernel<4, false>: no control wave, every wave keeps its set"""
    eng = bpp_amd.Engine(0)
    data = synth.make_dataset(40, 300, 4, "jc69", 1, seed=140)
    host = hostdrv.hip_driver(eng, tape.make_engine_loci(eng, data), data, seed=5)
    _setup(host, 4, program=False, bpp=False)
    dev = _device(eng, data, 4, DENSE | COUNTERS, program=False, bpp=False)
    _against_host(dev, host, 40, gibbs=False)
    assert "sets change waves: no" in capfd.readouterr().err
    host.close(); dev.close(); eng.close()


def test_eight_taxa_keep_the_identity_schedule(capfd):
    """iter_kernel<8, true, true>: 16 lanes a locus, three waves of loci a workgroup"""
    eng = bpp_amd.Engine(0)
    data = synth.make_dataset(20, 300, 8, "jc69", 1, seed=120)
    host = hostdrv.hip_driver(eng, tape.make_engine_loci(eng, data), data, seed=5)
    _setup(host, 8)
    dev = _device(eng, data, 8, DENSE | COUNTERS)
    _against_host(dev, host, 20)
    assert "sets change waves: no" in capfd.readouterr().err
    host.close(); dev.close(); eng.close()


def test_a_launch_that_gives_up_between_hand_overs_is_run_again(tmp_path):
    """inject=2: the second launch gives up at its first exchange — the sets have changed waves in its sweep by then —
    and stores nothing; the iterations run again from the trees, the streams and the holders the first launch left in HBM.  The
    chain is the host driver's, and to the bit that of a device run without the time-out."""
    eng = bpp_amd.Engine(0)
    nloci = 40
    data = synth.make_dataset(nloci, 300, 4, "jc69", 1, seed=140)
    host = hostdrv.hip_driver(eng, tape.make_engine_loci(eng, data), data, seed=5)
    _setup(host, 4)
    dev = _device(eng, data, 4, DENSE, dict(inject=2))
    _against_host(dev, host, nloci)
    got = _dump(dev, nloci, tmp_path / "inject")
    dev.close()
    ref = _device(eng, data, 4, DENSE)
    for chunk in CHUNKS:
        ref.iterate(chunk)
    want = _dump(ref, nloci, tmp_path / "plain")
    for k in want:
        assert (got[k] == want[k]).all(), k
    host.close(); ref.close(); eng.close()
