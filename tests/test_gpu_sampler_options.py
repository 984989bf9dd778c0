"""The environment and bpp_amd.Sampler's arguments are the same thing (include/bpp_amd.h: bpa_sampler_options): a sampler made
with a variable set around a plain Sampler(...) call and one made with the argument are of the same kind and, after 3
iterations, hold the same taus, thetas, trees and counters and have made the same launches, to the bit.  8 JC69 loci of 4 tips
and 300 sites (tests/test_invgamma_abi.py's set): they fit the persistent kernel, so every forced implementation changes the
outcome.  The only test besides tests/test_sampler_options.py that sets one of the sampler's variables."""
import numpy as np
import pytest

import bpp_amd
from bpp_amd import synth
import shapes
import tape

pytestmark = pytest.mark.gpu

# environment, arguments, moves, the kind both must report
CASES = {
    "automatic": ({}, {}, "uniform", "persistent"),
    "sweep": (dict(BPA_SMP_V1="1"), dict(implementation="sweep"), "uniform", "sweep"),
    "generic": (dict(BPA_SMP_GENERIC="1"), dict(implementation="generic"), "uniform", "generic"),
    "generic-chain-off": (dict(BPA_SMP_GENERIC="1", BPA_GS_CHAIN="0"), dict(implementation="generic", chain=False), "uniform", "generic"),
    "generic-chain-on": (dict(BPA_SMP_GENERIC="1", BPA_GS_CHAIN="1"), dict(implementation="generic", chain=True), "uniform", "generic"),
    "generic-program-host-decisions": (dict(BPA_SMP_GENERIC="1", BPA_GS_HOSTDEC="1"), dict(implementation="generic", host_decisions=True),
                                       "program", "generic"),
    "big": (dict(BPA_SMP_BIG="1"), dict(implementation="big"), "uniform", "big"),
}
COMPOSITE = {"composite-allowed": ({}, {}), "composite-refused": (dict(BPA_SMP_NO_COMPOSITE="1"), dict(composite=False))}


def jc4():
    data = synth.make_dataset(8, 300, 4, "jc69", 1, seed=5)
    stree = synth.species_tree_arrays(4)
    return shapes._case("jc4", data, [list(range(4))] * 8, stree, None, theta_prior=(2.0, 1000.0, 0.001), finetune=(0.003, 0.005, 0.0008, 0.2))


def run(eng, c, moves, env, args, monkeypatch):
    """kind and the state after 3 iterations, or the refusal's message"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        smp = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, c["data"]), c["data"], seed=3, **args)
    except bpp_amd.BpaError as ex:
        return str(ex)
    finally:
        for k in env:
            monkeypatch.delenv(k)
    shapes.configure(smp, c, moves)
    smp.initialize()
    smp.iterate(3)
    s = smp.summary()
    out = dict(kind=smp.kind(), taus=list(smp.taus()), thetas=list(smp.thetas()), trees=[smp.tree(i) for i in range(len(c["data"]))],
               counters=(s["proposals"], s["accepted"]) + ((smp.gibbs_counters(),) if moves == "program" else ()), launches=s["launches"])
    smp.close()
    return out


def same(a, b):
    assert type(a) is type(b)
    if isinstance(a, str):
        assert a == b
        return
    for key in ("kind", "taus", "thetas", "counters", "launches"):
        assert a[key] == b[key], key
    for i, (x, y) in enumerate(zip(a["trees"], b["trees"])):
        assert sorted(x) == sorted(y)
        for key in x:
            assert np.array_equal(np.asarray(x[key]), np.asarray(y[key])), (i, key)


@pytest.mark.parametrize("name", list(CASES))
def test_a_variable_and_its_argument_make_the_same_sampler(name, monkeypatch):
    env, args, moves, kind = CASES[name]
    c = jc4()
    eng = bpp_amd.Engine(0)
    by_env, by_arg = run(eng, c, moves, env, {}, monkeypatch), run(eng, c, moves, {}, args, monkeypatch)
    same(by_env, by_arg)
    assert by_arg["kind"] == kind
    assert by_arg["taus"] != list(c["stree"][1]) and by_arg["counters"][1] > 0            # (the chain moved)
    eng.close()


@pytest.mark.parametrize("name", list(COMPOSITE))
def test_the_composite_allowed_and_refused_by_variable_and_by_argument(name, monkeypatch):
    """shapes.case("composite-64-65"): 64- and 65-pattern JC69 loci and six GTR+Gamma4 loci — a composite, or without one the plain
    sampler's refusal of one- and several-category loci together"""
    env, args = COMPOSITE[name]
    c = shapes.case("composite-64-65")
    eng = bpp_amd.Engine(0)
    by_env, by_arg = run(eng, c, "uniform", env, {}, monkeypatch), run(eng, c, "uniform", {}, args, monkeypatch)
    same(by_env, by_arg)
    if name == "composite-allowed":
        assert by_arg["kind"] == "composite"
    else:
        assert "all be JC69 with one rate category or all have several categories" in by_arg      # (the plain sampler's refusal, as ever)
    eng.close()
