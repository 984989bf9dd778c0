"""The closed-form models' parameter moves: the interface.  a00_set_subst_kind / a00_set_qrates_prior (include/bpp_amd_host.h,
libbpp_amd_host.so), bpa_sampler_set_qrates_prior / bpa_sampler_subst_steps (include/bpp_amd.h, libbpp_amd.so, bpp_amd.Sampler),
the step table and the prior's term (include/bpp_amd_priors.h) — exported, declared, bound; the table as compiled against
the issue's table written out by hand (tests/closedform.py); the model constants; the data generator's new models."""
import ctypes
import os
import re

import numpy as np
import pytest

import bpp_amd
from bpp_amd import api, build, synth
import closedform as CF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_symbols_are_exported_declared_and_bound():
    L = bpp_amd.lib()
    src = header("bpp_amd.h")
    assert re.search(r"\bint\s+bpa_sampler_set_qrates_prior\s*\(\s*bpa_sampler_t\s*\*\s*,\s*const\s+double\s+a\[6\]\s*\)\s*;", src)
    assert re.search(r"\bint\s+bpa_sampler_subst_steps\s*\(\s*bpa_sampler_t\s*\*\s*,\s*unsigned\s*\*\s*freq_steps\s*,\s*unsigned\s*\*\s*qrate_steps\s*\)\s*;", src)
    for fn in ("bpa_sampler_set_qrates_prior", "bpa_sampler_subst_steps"):
        assert hasattr(L, fn) and fn in api.EXPORTED, fn
        assert getattr(L, fn).restype is ctypes.c_int
    assert len(L.bpa_sampler_set_qrates_prior.argtypes) == 2 and len(L.bpa_sampler_subst_steps.argtypes) == 3
    assert callable(bpp_amd.Sampler.set_qrates_prior) and callable(bpp_amd.Sampler.subst_steps)
    # the existing signatures stay
    assert re.search(r"\bint\s+bpa_sampler_set_subst_model\s*\(\s*bpa_sampler_t\s*\*\s*,\s*unsigned\s+i\s*,\s*const\s+double\s*\*\s*freqs\s*,\s*const\s+double\s*\*\s*qrates\s*,\s*double\s+alpha\s*\)\s*;", src)
    H = ctypes.CDLL(build.HOST_OUT)
    hsrc = header("bpp_amd_host.h")
    assert re.search(r"\bint\s+a00_set_subst_kind\s*\(\s*a00_driver_t\s*\*\s*,\s*unsigned\s+i\s*,\s*int\s+model\s*\)\s*;", hsrc)
    assert re.search(r"\bint\s+a00_set_qrates_prior\s*\(\s*a00_driver_t\s*\*\s*,\s*const\s+double\s+a\[6\]\s*\)\s*;", hsrc)
    for fn in ("a00_set_subst_kind", "a00_set_qrates_prior", "a00_qrates_prior_piece", "a00_subst_table"):
        assert hasattr(H, fn), fn
    psrc = header("bpp_amd_priors.h")
    for fn in ("a00_subst_qrates", "a00_subst_ref", "a00_subst_steps", "a00_subst_entry", "a00_qrates_prior_lnratio"):
        assert len(re.findall(r"static inline A00_HD \w+ " + fn + r"\s*\(", psrc)) == 1, fn


def test_model_constants():
    src = header("bpp_amd.h")
    for name, v in (("K80", 1), ("F81", 2), ("HKY", 3), ("T92", 4), ("TN93", 5), ("F84", 6)):
        assert re.search(r"#define\s+BPA_DNA_MODEL_%s\s+%d\b" % (name, v), src)
        assert getattr(bpp_amd, "MODEL_" + name) == v == CF.MODELS[name.lower()]
    assert bpp_amd.MODEL_GTR == 7 and bpp_amd.MODEL_JC69 == 0


def _table(model, which, step):
    H = CF.lib()
    H.a00_subst_table.argtypes = [ctypes.c_int]*3 + [ctypes.POINTER(ctypes.c_int)]*3
    e, r, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    nq = H.a00_subst_table(model, which, step, ctypes.byref(e), ctypes.byref(r), ctypes.byref(n))
    return nq, e.value, r.value, n.value


@pytest.mark.parametrize("model", list(CF.TABLE))
def test_step_table_as_compiled(model):
    """entries, reference entry, the entries the steps move in order and the number of frequency steps: the issue's table"""
    nq, ref, moved, nfreq = CF.TABLE[model]
    for code in ([CF.MODELS[model]] + ([100] if model == "gtr" else [])):         # (100: the device's tag of a GTR locus)
        got = [_table(code, 2, s) for s in range(-1, 7)]
        assert got[0][0] == nq
        assert got[0][3] == len(moved)
        assert [g[1] for g in got] == [-1] + list(moved) + [-1]*(7 - len(moved))
        if ref is not None:
            assert got[0][2] == ref and ref not in moved and ref < nq
        fr = [_table(code, 1, s) for s in range(-1, 5)]
        assert fr[0][3] == nfreq and fr[0][2] == 3
        assert [g[1] for g in fr] == [-1] + list(range(nfreq)) + [-1]*(5 - nfreq)
    assert _table(0, 1, 0)[1] == -1 and _table(0, 2, 0)[1] == -1 and _table(0, 2, 0)[0] == 0      # JC69 moves nothing


def test_host_driver_refuses_bad_kinds_and_priors():
    data = synth.make_dataset(2, 60, 4, "gtr", 4, seed=3)
    import hostdrv
    drv = CF.KindDriver(hostdrv.prior_driver(data, seed=1))
    assert not drv.try_set_subst_kind(2, "hky") and not drv.try_set_subst_kind(0, 0) and not drv.try_set_subst_kind(0, 8)
    assert all(drv.try_set_subst_kind(0, m) for m in CF.TABLE)
    assert not drv.try_set_qrates_prior([1, 1, 0, 1, 1, 1]) and not drv.try_set_qrates_prior([1, 1, 1, 1, 1, float("inf")])
    assert not drv.try_set_qrates_prior([1, 1, 1, float("nan"), 1, 1])
    assert drv.try_set_qrates_prior(CF.PROGRAM_PRIOR) and drv.try_set_qrates_prior(CF.FLAT_PRIOR)
    drv.close()


def test_synth_makes_the_closed_form_models_and_leaves_the_old_calls_alone():
    """every new model gives 4-state loci that carry the model's own entries; a call without the new argument draws what it
    drew (the stream of the generator is used in the same order: the GTR set of another test's seed, three sequences pinned)"""
    for m in CF.CLOSED:
        d = synth.make_dataset(3, 80, 4, m, 2, seed=11, kappa=3.0)
        assert len(d) == 3 and all(x["model"] == m and x["states"] == 4 and len(x["exch"]) == 6 and len(x["freqs"]) == 4 for x in d)
        assert abs(sum(d[0]["freqs"]) - 1) < 1e-15
        if m == "k80":
            assert list(d[0]["freqs"]) == [0.25]*4
        nq = CF.TABLE[m][0]
        assert list(d[0]["exch"][nq:]) == [1.0]*(6 - nq)
    q, g = synth.closed_form_rates("hky", 3.0, [0.3, 0.2, 0.2, 0.3])
    assert list(q) == [1, 3, 1, 1, 1, 1] and list(g) == [1, 3, 1, 1, 3, 1]
    q, g = synth.closed_form_rates("f84", 2.0, [0.3, 0.2, 0.2, 0.3])
    assert list(q[:2]) == [2, 1] and g[1] == 1 + 2/0.5 and g[4] == 1 + 2/0.5
    a = synth.make_dataset(2, 100, 4, "gtr", 4, seed=3)
    b = synth.make_dataset(2, 100, 4, "gtr", 4, 0.5, None, 3)
    assert [x["seqs"] for x in a] == [x["seqs"] for x in b] and a[0]["seqs"][0].startswith("ACCGT")
    # same alignments under another ratio differ: kappa reaches the simulation
    h2, h9 = synth.make_dataset(2, 200, 4, "hky", 1, seed=3), synth.make_dataset(2, 200, 4, "hky", 1, seed=3, kappa=9.0)
    assert [x["seqs"] for x in h2] != [x["seqs"] for x in h9]
