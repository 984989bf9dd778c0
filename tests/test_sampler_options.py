"""bpa_sampler_options_from_env (include/bpp_amd.h): the one place the sampler code reads the process environment.  Host-only:
no device.  (That a sampler made through the environment and one made through the argument are the same sampler:
tests/test_gpu_sampler_options.py.)"""
import ctypes as C

import pytest

import bpp_amd

VARIABLES = ("BPA_SMP_BIG", "BPA_SMP_GENERIC", "BPA_SMP_V1", "BPA_SMP_NO_COMPOSITE", "BPA_GS_CHAIN", "BPA_GS_HOSTDEC", "BPA_SMP_DBG",
             "BPA_SMP_TRACE", "BPA_SMP_INJECT", "BPA_GS_DIFF", "A00_DECLOG")
AUTO, SWEEP, GENERIC, BIG = -1, 0, 1, 4                    # BPA_SAMPLER_AUTO, _SWEEP, _GENERIC, _BIG
DEFAULTS = dict(size=C.sizeof(bpp_amd.SamplerOptions), implementation=AUTO, composite=1, chain=-1, host_decisions=0, debug=0,
                launch_times=0, inject=0, inject_wg0=0, diff=0, decision_log=0)


def options(monkeypatch, **env):
    """the struct's fields as bpa_sampler_options_from_env fills them with exactly `env` set"""
    for v in VARIABLES:
        monkeypatch.delenv(v, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    o = bpp_amd.SamplerOptions(size=0, implementation=77, composite=77, chain=77, host_decisions=77, debug=77, launch_times=77,
                               inject=77, inject_wg0=77, diff=77, decision_log=77)            # (every field is written)
    bpp_amd.lib().bpa_sampler_options_from_env(C.byref(o))
    return {name: getattr(o, name) for name, _ in bpp_amd.SamplerOptions._fields_}


def test_the_struct_is_the_header_s():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bpp_amd.h")).read()
    body = re.search(r"typedef struct bpa_sampler_options\s*\{(.*?)\}\s*bpa_sampler_options;", src, re.S).group(1)
    fields = [n for decl in body.split(";") if decl.strip() for n in re.sub(r"^\s*(unsigned|int|long)\s", "", decl).replace(" ", "").split(",")]
    assert fields == [name for name, _ in bpp_amd.SamplerOptions._fields_] == list(DEFAULTS)


def test_a_clean_environment_gives_the_documented_defaults(monkeypatch):
    assert options(monkeypatch) == DEFAULTS


@pytest.mark.parametrize("env,changed", [
    (dict(BPA_SMP_BIG="1"), dict(implementation=BIG)),
    (dict(BPA_SMP_GENERIC="1"), dict(implementation=GENERIC)),
    (dict(BPA_SMP_V1="1"), dict(implementation=SWEEP)),
    (dict(BPA_SMP_NO_COMPOSITE="1"), dict(composite=0)),
    (dict(BPA_GS_CHAIN="0"), dict(chain=0)),
    (dict(BPA_GS_CHAIN="1"), dict(chain=1)),
    (dict(BPA_GS_HOSTDEC="1"), dict(host_decisions=1)),
    (dict(BPA_SMP_DBG="4112"), dict(debug=4112)),
    (dict(BPA_SMP_TRACE="1"), dict(launch_times=1)),
    (dict(BPA_SMP_INJECT="2"), dict(inject=2, inject_wg0=0)),
    (dict(BPA_SMP_INJECT="2,w"), dict(inject=2, inject_wg0=1)),
    (dict(BPA_GS_DIFF="1"), dict(diff=1)),
    (dict(A00_DECLOG="1"), dict(decision_log=1)),
    # several implementations asked for: big, then generic, then one launch per step
    (dict(BPA_SMP_BIG="1", BPA_SMP_GENERIC="1", BPA_SMP_V1="1"), dict(implementation=BIG)),
    (dict(BPA_SMP_GENERIC="1", BPA_SMP_V1="1"), dict(implementation=GENERIC)),
], ids=lambda v: "+".join(f"{k}={x}" for k, x in v.items()) if isinstance(next(iter(v.values())), str) else None)
def test_each_variable_changes_its_own_field_and_no_other(env, changed, monkeypatch):
    assert options(monkeypatch, **env) == dict(DEFAULTS, **changed)
    assert changed.items() - DEFAULTS.items()                  # (and that is not the default)
