"""The inverse-gamma priors' interface: bpa_sampler_set_prior_kinds (include/bpp_amd.h, libbpp_amd.so, bpp_amd.Sampler),
a00_set_prior_kinds (include/bpp_amd_host.h, libbpp_amd_host.so) and the prior families' arithmetic (include/bpp_amd_priors.h,
part of bpp_amd_host.h) — exported, declared, bound; the host driver's default; and, on a GPU, what the call refuses."""
import ctypes
import os
import re

import numpy as np
import pytest

import bpp_amd
from bpp_amd import api, build, synth
import hostdrv
import invgamma as IG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_symbols_are_exported_declared_and_bound():
    L = bpp_amd.lib()
    src = header("bpp_amd.h")
    assert re.search(r"\bint\s+bpa_sampler_set_prior_kinds\s*\(\s*bpa_sampler_t\s*\*\s*,\s*int\s+theta_kind\s*,\s*int\s+tau_kind\s*\)\s*;", src)
    assert re.search(r"#define\s+BPA_PRIOR_GAMMA\s+0\b", src) and re.search(r"#define\s+BPA_PRIOR_INVGAMMA\s+1\b", src)
    assert hasattr(L, "bpa_sampler_set_prior_kinds") and "bpa_sampler_set_prior_kinds" in api.EXPORTED
    assert L.bpa_sampler_set_prior_kinds.restype is ctypes.c_int and len(L.bpa_sampler_set_prior_kinds.argtypes) == 3
    assert callable(bpp_amd.Sampler.set_prior_kinds) and bpp_amd.Sampler.PRIOR_KINDS == {"gamma": 0, "invgamma": 1}
    H = ctypes.CDLL(build.HOST_OUT)
    hsrc = header("bpp_amd_host.h")
    assert re.search(r"\bvoid\s+a00_set_prior_kinds\s*\(\s*a00_driver_t\s*\*\s*,\s*int\s+theta_kind\s*,\s*int\s+tau_kind\s*\)\s*;", hsrc)
    assert hasattr(H, "a00_set_prior_kinds") and hasattr(H, "a00_prior_piece")
    assert '#include "bpp_amd_priors.h"' in hsrc
    psrc = header("bpp_amd_priors.h")
    assert re.search(r"#define\s+A00_PRIOR_GAMMA\s+0\b", psrc) and re.search(r"#define\s+A00_PRIOR_INVGAMMA\s+1\b", psrc)
    for fn in ("a00_theta_prior_lnratio", "a00_tau_prior_lnratio", "a00_mix_tau_prior_lnratio", "a00_theta_conditional_kind", "a00_theta_lnacc_kind"):
        assert re.search(r"static inline A00_HD \w+ " + fn + r"\s*\(\s*int kind\b", psrc), fn


def _driver(seed=3, nloci=4):
    parent, tau0, thetas = synth.species_tree_arrays(4)
    sp = [0, 0, 1, 1, 2, 2, 3, 3]
    rng = np.random.default_rng(70)
    data = []
    for _ in range(nloci):
        l, r, t, rt = synth.msc_start_tree(sp, parent, tau0, thetas, rng)
        data.append(dict(seqs=["A"]*8, left=l, right=r, times=t, root=rt))
    drv = IG.KindDriver(hostdrv.prior_driver(data, seed=seed))
    return drv, (parent, tau0, thetas), [sp]*nloci


@pytest.mark.parametrize("moves", ["uniform", "program"])
def test_host_driver_default_is_gamma_to_the_bit(moves):
    """a driver that never calls a00_set_prior_kinds, one that asks for gamma / gamma and one that passes values other than the
    two kinds walk the same trajectory (==); inverse gamma walks another"""
    runs = []
    for kinds in (None, ("gamma", "gamma"), (7, -1), ("invgamma", "gamma"), ("gamma", "invgamma")):
        drv, stree, species = _driver()
        IG.configure(drv, stree, species, moves, theta_prior=(2.0, 1000.0, 0.0006), tau_prior=(3.0, 3.0/stree[1][-1]),
                     finetune=(0.003, 0.005, 0.0006, 0.2), kinds=kinds)
        drv.initialize()
        for _ in range(30):
            drv.iterate()
        runs.append((drv.counters(), drv.taus(), drv.thetas(), [drv.tree(i) for i in range(4)]))
        drv.close()
    assert runs[0] == runs[1] == runs[2]
    assert runs[3] != runs[0] and runs[4] != runs[0] and runs[3] != runs[4]


# ---- what bpa_sampler_set_prior_kinds refuses (a sampler needs a device)
def _sampler(eng, data, implementation=None):
    import tape
    smp = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, data), data, seed=3, implementation=implementation)
    parent, tau0, thetas = synth.species_tree_arrays(len(data[0]["seqs"]))
    smp.set_species_tree(parent, tau0, thetas)
    smp.set_tau_prior(3.0, 2.0*tau0[-1])
    smp.set_theta_prior(3.0, 0.004, 0.001)
    return smp


@pytest.mark.gpu
def test_what_set_prior_kinds_refuses():
    eng = bpp_amd.Engine(0)
    jc4 = synth.make_dataset(8, 300, 4, "jc69", 1, seed=5)
    way_out = "the persistent kernel has the gamma priors only: implementation = BPA_SAMPLER_GENERIC or BPA_SAMPLER_SWEEP in the options at creation"
    # loci that fit the persistent kernel get it (alone: BPA_SAMPLER_PERSISTENT; with an all-reduce callback: BPA_SAMPLER_HYBRID)
    smp = _sampler(eng, jc4)
    with pytest.raises(bpp_amd.BpaError, match=way_out):
        smp.set_prior_kinds("invgamma", "invgamma")
    with pytest.raises(bpp_amd.BpaError, match=way_out):
        smp.set_prior_kinds("gamma", "invgamma")
    smp.set_allreduce(lambda p, n, st: True, None, 0)
    with pytest.raises(bpp_amd.BpaError, match="gamma priors only"):
        smp.set_prior_kinds("invgamma", "invgamma")
    assert smp.kind() == "hybrid"
    smp.close()
    # ... and the message's two ways out are ways out
    for kind in ("generic", "sweep"):
        smp = _sampler(eng, jc4, kind)
        smp.set_prior_kinds("invgamma", "invgamma")
        # a kind other than the two
        for bad in ((2, 0), (0, -1), (1, 7)):
            with pytest.raises(bpp_amd.BpaError, match="BPA_PRIOR_GAMMA or BPA_PRIOR_INVGAMMA"):
                smp.set_prior_kinds(*bad)
        with pytest.raises(bpp_amd.BpaError, match="'gamma' or 'invgamma'"):
            smp.set_prior_kinds("lognormal", "gamma")
        # installing an exchange afterwards
        with pytest.raises(bpp_amd.BpaError, match="gamma priors only"):
            smp.set_allreduce(lambda p, n, st: True, None, 0)
        smp.initialize()
        assert smp.kind() == kind
        # a call after initialize
        with pytest.raises(bpp_amd.BpaError, match="before bpa_sampler_initialize"):
            smp.set_prior_kinds("gamma", "gamma")
        smp.iterate(2)
        smp.close()
    # a sampler with an all-reduce callback installed, whatever its kind
    smp = _sampler(eng, jc4, "generic")
    smp.set_allreduce(lambda p, n, st: True, None, 0)
    with pytest.raises(bpp_amd.BpaError, match="several ranks have the gamma priors only"):
        smp.set_prior_kinds("invgamma", "gamma")
    smp.close()
    # loci of several kinds (BPA_SAMPLER_COMPOSITE)
    import shapes
    c = shapes.case("composite-64-65")
    import tape
    comp = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, c["data"]), c["data"], seed=3)
    with pytest.raises(bpp_amd.BpaError, match="loci of several kinds"):
        comp.set_prior_kinds("invgamma", "invgamma")
    shapes.configure(comp, c, "uniform")
    assert comp.kind() == "composite"
    comp.close()
    eng.close()
