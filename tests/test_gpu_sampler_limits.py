"""The device samplers at their pattern- and tip-count limits, on loci of exact shape (tests/shapes.py; the same sets under
the host driver on the reference's locus API: tests/test_host_driver_limits.py).

 * persistent kernel (csrc/sweep2.hpp), 4-tip form: 1 .. 64 patterns per locus — up to eight passes of the pattern loop,
   waves that close on patterns, a wave of one 64-pattern locus, idle lane groups, non-zero first pattern slots; 8-tip form:
   1 .. 64 patterns, up to four passes; loci of 2, 3, 4, 5, 7 and 8 tips in one sampler;
 * the same lists on the one-launch-per-step path (csrc/sampler.hpp), bit for bit;
 * 65 patterns: the generic sampler takes the set, or the composite the 65-pattern loci;
 * generic sampler (csrc/gsampler*.hpp) at 16 tips (31 nodes in 32-bit node-set masks), at 252, 255 and 248 lanes, 12 and 16
   tips side by side; what it refuses: 256 lanes;
 * big-tree sampler (csrc/bigsampler*.hpp) at 17 and at 64 tips, with and without scale buffers; what it refuses: 65 tips.

Every case: the trajectory of the C host driver on the same library for 4 iterations (walk() of tests/test_gpu_gsampler.py),
then on a fresh sampler the whole state against a CPU recompute (grow() of tests/test_gpu_state_invariants.py: check_state
after 1, 7 and 200 iterations — the second chunk is a multi-iteration launch).  The bars are walk()'s and check_state's own.
Measured differences: the table in tests/test_gpu_state_invariants.py.
"""
import numpy as np
import pytest

import bpp_amd
from bpp_amd import synth
import hostdrv
import tape
import shapes
from invariants import oracle_locus
from test_gpu_gsampler import walk
from test_gpu_state_invariants import grow

pytestmark = pytest.mark.gpu
MOVES = ["uniform", "program"]


def sampler(eng, c, moves, seed, scaling=False, **options):
    loci = tape.make_engine_loci(eng, c["data"], scaling)
    dev = bpp_amd.Sampler(eng, loci, c["data"], seed=seed, **options)
    shapes.configure(dev, c, moves)
    return dev, loci


def walk_and_grow(name, moves, chunks=(1, 7, 200), scaling=False, tag="", **options):
    """-> the sampler after grow (open, with its engine: the caller closes both)"""
    c = shapes.case(name)
    n = len(c["data"])
    eng = bpp_amd.Engine(0)
    host = hostdrv.hip_driver(eng, tape.make_engine_loci(eng, c["data"], scaling), c["data"], seed=29, scaling=scaling)
    shapes.configure(host, c, moves, host=True)
    dev, _ = sampler(eng, c, moves, 29, scaling, **options)
    # (the program's moves go through libm's log / sqrt / lgamma on both sides: the tolerance the existing walks give them)
    walk(host, dev, 4, n, **(dict(tol=1e-9) if moves == "program" else {}))
    assert dev.kind() == c["kind"]
    if c["subst"]:
        for i in range(n):
            (fh, qh, ah), (fd, qd, ad) = host.get_subst_model(i), dev.get_subst_model(i)
            assert np.allclose(fd, fh, rtol=1e-11, atol=0) and np.allclose(qd, qh, rtol=1e-11, atol=0) and abs(ad - ah) <= 1e-11 * abs(ah), i
    host.close(); dev.close()
    dev, loci = sampler(eng, c, moves, 31, scaling, **options)
    dev.initialize()
    assert dev.kind() == c["kind"]
    grow(f"limits-{name}-{moves}{tag}", dev, chunks, c["stree"][1], c["stree"][2], data=c["data"], species_parent=c["stree"][0], loci=loci,
         tip_species=c["species"], scaling=scaling, subst=c["subst"] or None)
    return dev, eng


# ------------------------------------------------------------------ a, b: the persistent kernel
def test_the_lists_reach_the_packing_s_edges():
    """sampler_upload_v2's `cnt == LPW || used + np > 64` and sampler_upload's `used + np > BS || ntask == TPB` on the two lists"""
    shapes.check_lists()


@pytest.mark.parametrize("moves", MOVES)
@pytest.mark.parametrize("name", ["persistent-4", "persistent-8"])
def test_persistent_kernel_at_its_pattern_limits(name, moves):
    c = shapes.case(name)
    assert [len(d["weights"]) for d in c["data"]] == list(shapes.COUNTS4 if name == "persistent-4" else shapes.COUNTS8)
    dev, eng = walk_and_grow(name, moves)
    dev.close(); eng.close()


@pytest.mark.parametrize("moves", MOVES)
def test_persistent_kernel_with_loci_of_2_to_8_tips_in_one_sampler(moves):
    """two species with 1+1, 2+1, 2+2, 3+2, 4+3 and 4+4 sequences, at 20 and at 40 patterns: the library takes them in one sampler
    (the 8-tip form); the tip populations' thetas move"""
    c = shapes.case("persistent-mixed-tips")
    assert sorted({len(s) for s in c["species"]}) == [2, 3, 4, 5, 7, 8] and {len(d["weights"]) for d in c["data"]} == {20, 40}
    dev, eng = walk_and_grow("persistent-mixed-tips", moves)
    assert all(a != b for a, b in zip(dev.thetas()[:2], c["stree"][2][:2]))
    dev.close(); eng.close()


# ------------------------------------------------------------------ c: one launch per step
@pytest.mark.parametrize("name", ["persistent-4", "persistent-8", "persistent-mixed-tips"])
def test_persistent_kernel_equals_one_launch_per_step_at_the_limits(name):
    """what tests/test_gpu_sampler.py::test_persistent_kernel_equals_one_launch_per_step asserts, on the shaped lists: trees,
    taus, thetas and counters bit for bit over 6 iterations in chunks of 1 and 4"""
    c = shapes.case(name)
    eng = bpp_amd.Engine(0)
    new, _ = sampler(eng, c, "uniform", 11)
    new.initialize()
    old, _ = sampler(eng, c, "uniform", 11, implementation="sweep")
    old.initialize()
    assert new.kind() == "persistent" and old.kind() == "sweep"
    for it, n in enumerate((1, 4, 1)):
        new.iterate(n); old.iterate(n)
        assert new.taus() == old.taus() and new.thetas() == old.thetas(), it
        a, b = new.summary(), old.summary()
        assert (a["proposals"], a["accepted"]) == (b["proposals"], b["accepted"]), it
        assert a["launches"] < b["launches"]
    assert new.taus() != list(c["stree"][1])
    for i in range(len(c["data"])):
        x, y = new.tree(i), old.tree(i)
        for key in ("left", "right", "parent", "clv", "pmat", "pop", "time"):
            assert list(x[key]) == list(y[key]), (i, key)
        assert x["root"] == y["root"] and x["lnl"] == y["lnl"] and x["logpr"] == y["logpr"], i
    new.close(); old.close(); eng.close()


# ------------------------------------------------------------------ d: 65 patterns
@pytest.mark.parametrize("moves", MOVES)
def test_one_locus_of_65_patterns_hands_the_set_to_the_generic_sampler(moves):
    c = shapes.case("handover-65")
    counts = [len(d["weights"]) for d in c["data"]]
    assert counts.count(65) == 1 and sum(a != b for a, b in zip(counts, shapes.COUNTS4)) == 1
    dev, eng = walk_and_grow("handover-65", moves)
    dev.close(); eng.close()


def test_64_and_65_pattern_loci_in_turns_with_gtr_loci_make_a_composite():
    c = shapes.case("composite-64-65")
    counts = [len(d["weights"]) for d in c["data"] if d["model"] == "jc69"]
    assert counts == [64, 65] * 64 and sum(d["model"] == "gtr" for d in c["data"]) == 6
    dev, eng = walk_and_grow("composite-64-65", "uniform")
    dev.close(); eng.close()


# ------------------------------------------------------------------ e: the generic sampler
@pytest.mark.parametrize("chain", [0, 1])
@pytest.mark.parametrize("moves", MOVES)
@pytest.mark.parametrize("name", ["generic-16-jc", "generic-16-gtr-g4", "generic-16-gtr-g3", "generic-16-gtr-g8", "generic-12-and-16"])
def test_generic_sampler_at_its_limits(name, moves, chain):
    """16 tips; JC69 at 1, 64, 200 and 255 patterns; GTR+Gamma4 at 63 patterns (252 lanes) with the parameter moves; GTR with 3
    categories at 85 (255 lanes), with 8 at 31 (248); 12 and 16 tips in one sampler.  The per-locus steps as a launch each
    (chain=0) and as one launch (1)"""
    c = shapes.case(name)
    lanes = max(len(d["weights"]) * d["rate_cats"] for d in c["data"])
    assert max(len(s) for s in c["species"]) == 16 and lanes == {"generic-16-jc": 255, "generic-16-gtr-g4": 252, "generic-16-gtr-g3": 255,
                                                                 "generic-16-gtr-g8": 248, "generic-12-and-16": 100}[name]
    dev, eng = walk_and_grow(name, moves, tag=f"-chain{chain}", chain=chain)
    if c["subst"]:
        assert any(dev.get_subst_model(i)[2] != 0.5 for i in range(len(c["data"])))
    dev.close(); eng.close()


def test_generic_sampler_refuses_256_lanes():
    st8 = synth.species_tree_arrays(8)
    rng = np.random.default_rng(3)
    msg = "< 256 patterns x categories"
    eng = bpp_amd.Engine(0)
    for tips in (9, 16):
        sp = ([k // 2 for k in range(16)])[:tips]
        mixed = [shapes.shaped_locus(sp, st8, 256, rng=rng), shapes.shaped_locus(sp, st8, 40, "gtr", 4, rng=rng)]
        with pytest.raises(bpp_amd.BpaError, match=msg):
            bpp_amd.Sampler(eng, tape.make_engine_loci(eng, mixed), mixed)
    sp = [k // 2 for k in range(16)]
    for tips in (8, 16):
        g64 = [shapes.shaped_locus(sp[:tips], st8, 64, "gtr", 4, rng=rng)]
        with pytest.raises(bpp_amd.BpaError, match=msg):
            bpp_amd.Sampler(eng, tape.make_engine_loci(eng, g64), g64)
    # one pattern fewer is taken
    ok = [shapes.shaped_locus(sp, st8, 255, rng=rng)]
    smp = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, ok), ok)
    smp.set_species_tree(*st8)
    smp.set_tip_species(0, sp)
    smp.initialize()
    assert smp.kind() == "generic"
    smp.close(); eng.close()


# ------------------------------------------------------------------ f: the big-tree sampler
@pytest.mark.parametrize("moves", MOVES)
@pytest.mark.parametrize("scaling", [False, True])
@pytest.mark.parametrize("name", shapes.BIG)
def test_big_tree_sampler_at_its_limits(name, scaling, moves):
    """17 tips (the first size beyond the generic sampler) and 64 (the last one admitted: 126 scale buffers), 3 loci at 30 and at
    300 patterns, with scale buffers and without"""
    c = shapes.case(name)
    assert len(c["data"]) == 3 and {len(s) for s in c["species"]} == {int(name.split("-")[1])}
    dev, eng = walk_and_grow(name, moves, chunks=(1, 3, 30), scaling=scaling, tag=f"-scal{int(scaling)}")
    # do the oracle's scale counters fire on these trees?  (either way is fine: the counters are compared with == above)
    fired = False
    for i, d in enumerate(c["data"]):
        t = dev.tree(i)
        ol = oracle_locus(d, None, None, True, None)
        ol.full_lnl([int(x) for x in t["left"]], [int(x) for x in t["right"]], [float(x) for x in t["time"]], int(t["root"]))
        fired = fired or any(s is not None and bool(np.any(s)) for s in ol.scaler)
    print(f"[invariants] limits-{name}-{moves}-scal{int(scaling)}: scale counters {'fire' if fired else 'all zero'} in the oracle's recompute")
    assert isinstance(fired, bool)
    dev.close(); eng.close()


def test_big_tree_sampler_refuses_65_tips():
    st8 = synth.species_tree_arrays(8)
    sp = [k // 9 for k in range(65)]
    data = [shapes.shaped_locus(sp, st8, 30, rng=np.random.default_rng(4))]
    eng = bpp_amd.Engine(0)
    with pytest.raises(bpp_amd.BpaError, match="<= 64 tips"):
        bpp_amd.Sampler(eng, tape.make_engine_loci(eng, data), data)
    with pytest.raises(bpp_amd.BpaError, match="<= 64 tips"):
        bpp_amd.Sampler(eng, tape.make_engine_loci(eng, data, True), data)
    eng.close()
