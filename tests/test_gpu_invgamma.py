"""Inverse-gamma theta / tau priors (BPP's defaults; bpa_sampler_set_prior_kinds) on the device samplers that have them — the
generic sampler (uniform windows; the program's moves decided on the device by gsm::gdec_kernel<.., 1> and, host_decisions, on
the host), the big-tree sampler (both move sets) and the one-launch-per-step sampler (implementation="sweep": smp::decide,
theta_sum_decide_kernel):

 * decision by decision against the C host driver with a00_set_prior_kinds on the same library (tests/invgamma.py: pair_walk);
 * prior-only runs on the device: every 1/theta and 1/tau_root gamma(a, b);
 * the program's own posterior under these priors (tests/golden/invgamma_posterior.json) on the generic sampler;
 * the persistent kernel refuses and runs on unchanged; gamma / gamma is the trajectory of a sampler that never heard of the
   call; the state after inverse-gamma runs passes tests/invariants.py's recompute.
CPU twin: tests/test_invgamma_host.py."""
import numpy as np
import pytest

import bpp_amd
from bpp_amd import synth
import hostdrv
import invariants
import invgamma as IG
import shapes
import tape
from test_invgamma_host import gold, dataset, setup, sample, compare, PRIOR_THETA, PRIOR_FT_THETA      # noqa: F401  (gold: the module's fixture)

pytestmark = pytest.mark.gpu

SP8 = [0, 0, 1, 1, 2, 2, 3, 3]                                         # 4 species x 2 sequences: every theta can hold a coalescence
_SETS = {}


def gtr8(n, theta=None):
    """n GTR+Gamma4 loci of 8 tips and about 25 patterns, their start trees from the species tree at `theta` (built once, never
    changed)"""
    if (n, theta) not in _SETS:
        _SETS[n, theta] = shapes.shaped_set(SP8, synth.species_tree_arrays(4, theta), [20 + k for k in range(n)], 85, model="gtr", rate_cats=4)
    return _SETS[n, theta]


def pair(eng, data, seed, env={}, scaling=False):
    """(host driver, device sampler) on two sets of engine loci; env: the sampler's options"""
    host = IG.KindDriver(hostdrv.hip_driver(eng, tape.make_engine_loci(eng, data, scaling), data, seed=seed, scaling=scaling))
    dev = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, data, scaling), data, seed=seed, **env)
    return host, dev


def moved(dev, stree):
    assert list(dev.taus()) != list(stree[1]) and list(dev.thetas()) != list(stree[2])


# ---------------------------------------------------------------- 5. generic sampler
@pytest.mark.parametrize("moves,env", [("uniform", {}), ("program", {}), ("program", dict(host_decisions=True))])
def test_generic_sampler_with_inverse_gamma_priors_equals_host_driver(moves, env):
    """6 GTR+Gamma4 loci of 8 tips (the 128-VGPR step kernel's path), 60 iterations"""
    stree = synth.species_tree_arrays(4)
    data = gtr8(6)
    eng = bpp_amd.Engine(0)
    host, dev = pair(eng, data, 37, env)
    program = moves == "program"
    for drv in (host, dev):
        IG.configure(drv, stree, [SP8]*6, moves, theta_prior=(3.0, 0.004, 0.0004 if program else 0.001),
                     finetune=(0.003, 0.005, 0.0004, 0.05) if program else (0.003, 0.005, 0.0008, 0.2))
    IG.pair_walk(host, dev, 60, 6, 1e-9 if program else 1e-12, program)
    assert dev.kind() == "generic"
    moved(dev, stree)
    dev.close(); host.close(); eng.close()


# ---------------------------------------------------------------- 6. big-tree sampler
@pytest.mark.parametrize("moves", ["uniform", "program"])
def test_big_tree_sampler_with_inverse_gamma_priors_equals_host_driver(moves):
    """3 loci of 17 tips (shapes.case('big-17-30'): 8 species), 40 iterations"""
    c = shapes.case("big-17-30")
    eng = bpp_amd.Engine(0)
    host, dev = pair(eng, c["data"], 23)
    program = moves == "program"
    for drv in (host, dev):
        IG.configure(drv, c["stree"], c["species"], moves, theta_prior=(3.0, 0.004, 0.001), finetune=c["finetune"])
    IG.pair_walk(host, dev, 40, 3, 1e-9 if program else 1e-12, program)
    assert dev.kind() == "big"
    assert list(dev.thetas()) != list(c["stree"][2])
    dev.close(); host.close(); eng.close()


def test_big_tree_sampler_forced_on_8_tip_loci_with_inverse_gamma_priors():
    stree = synth.species_tree_arrays(4)
    data = gtr8(6)
    eng = bpp_amd.Engine(0)
    host, dev = pair(eng, data, 41, dict(implementation="big"))
    for drv in (host, dev):
        IG.configure(drv, stree, [SP8]*6, "program", theta_prior=(3.0, 0.004, 0.0004), finetune=(0.003, 0.005, 0.0004, 0.05))
    IG.pair_walk(host, dev, 40, 6, 1e-9, True)
    assert dev.kind() == "big"
    moved(dev, stree)
    dev.close(); host.close(); eng.close()


# ---------------------------------------------------------------- 7. one launch per step
def test_one_launch_per_step_sampler_with_inverse_gamma_priors_equals_host_driver():
    """implementation="sweep": 8 JC69 loci of 4 tips, uniform windows, 60 iterations"""
    stree = synth.species_tree_arrays(4)
    data = synth.make_dataset(8, 300, 4, "jc69", 1, seed=47)
    eng = bpp_amd.Engine(0)
    host, dev = pair(eng, data, 53, dict(implementation="sweep"))
    for drv in (host, dev):
        IG.configure(drv, stree, None, "uniform")
    IG.pair_walk(host, dev, 60, 8, 1e-12, False)
    assert dev.kind() == "sweep"
    moved(dev, stree)
    dev.close(); host.close(); eng.close()


# ---------------------------------------------------------------- 8. prior only
@pytest.mark.parametrize("moves", ["uniform", "program"])
@pytest.mark.parametrize("which", ["generic", "big"])
def test_prior_only_run_on_the_device_leaves_the_inverse_gamma_priors(which, moves):
    """usedata = 0; generic: 12 loci of 8 tips, big-tree: 6 of them forced onto it; every move on, 500 + 2 000 x 3 iterations
    (tests/test_gpu_heredity.py, tests/test_gpu_bigsampler_scalars.py): every 1/theta ~ gamma(3, 2 theta_0), 1/tau_root ~
    gamma(3, 2 tau_0) — the host driver's check (tests/test_invgamma_host.py: its scale theta_0 = 0.01, its theta window and why), same step
    lengths and bars"""
    stree = synth.species_tree_arrays(4, PRIOR_THETA)
    n = 12 if which == "generic" else 6
    data = gtr8(n, PRIOR_THETA)
    eng = bpp_amd.Engine(0)
    eng.set_options(usedata=0, bfbeta=1.0)
    dev = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, data), data, seed=17, implementation="big" if which == "big" else None)
    theta_prior, tau_prior = (3.0, 2.0*PRIOR_THETA), (3.0, 2.0*stree[1][-1])
    IG.configure(dev, stree, [SP8]*n, moves, theta_prior=theta_prior + (PRIOR_FT_THETA,), tau_prior=tau_prior, finetune=(0.008, 0.008, 0.002, 0.5))
    dev.initialize()
    assert dev.kind() == which
    try:
        IG.prior_marginals(dev, dev.iterate, 500, 2000, 3, theta_prior, tau_prior, [True]*7)
    finally:
        eng.set_options(usedata=1, bfbeta=1.0)
    gp, ga = dev.gibbs_counters()
    assert (gp > 0 and ga == gp) if moves == "program" else (gp, ga) == (0, 0)
    dev.close(); eng.close()


# ---------------------------------------------------------------- 9. the program's posterior
@pytest.mark.parametrize("moves", ["uniform", "program"])
def test_generic_sampler_reproduces_bpp_posterior_under_inverse_gamma_priors(gold, moves):      # noqa: F811
    """implementation="generic" (these loci would fit the LDS kernels), 2 000 + 4 000 x 2 iterations, the fixture's bars"""
    data = dataset(gold)
    eng = bpp_amd.Engine(0)
    dev = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, data), data, seed=10, implementation="generic")
    setup(dev, gold, moves == "program")
    dev.initialize()
    assert dev.kind() == "generic"
    dev.iterate(2000)
    S = []
    for _ in range(4000):
        dev.iterate(2)
        S.append(sample(dev, False))
    compare(S, gold)
    dev.close(); eng.close()


# ---------------------------------------------------------------- 10. refusals and the default
def _state(smp, n):
    return list(smp.taus()), list(smp.thetas()), [smp.tree(i)["lnl"] for i in range(n)], smp.summary()["total_lnl"]


def test_the_persistent_kernel_refuses_and_runs_on_unchanged():
    stree = synth.species_tree_arrays(4)
    data = synth.make_dataset(40, 300, 4, "jc69", 1, seed=5)
    eng = bpp_amd.Engine(0)
    runs = []
    for ask in (False, True):
        smp = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, data), data, seed=2)
        IG.configure(smp, stree, None, "uniform", theta_prior=(2.0, 1000.0, 0.0005), tau_prior=(3.0, 3.0/stree[1][-1]), kinds=None)
        if ask:
            with pytest.raises(bpp_amd.BpaError, match="the persistent kernel has the gamma priors only: implementation = BPA_SAMPLER_GENERIC or BPA_SAMPLER_SWEEP in the options at creation"):
                smp.set_prior_kinds("invgamma", "invgamma")
        smp.initialize()
        smp.iterate(20)
        assert smp.kind() == "persistent"
        runs.append(_state(smp, 40))
        smp.close()
    assert runs[0] == runs[1]
    eng.close()


def test_gamma_gamma_is_the_trajectory_of_a_sampler_that_never_heard_of_the_call():
    stree = synth.species_tree_arrays(4)
    data = gtr8(6)
    eng = bpp_amd.Engine(0)
    runs = []
    for kinds in (None, ("gamma", "gamma"), ("invgamma", "invgamma")):
        smp = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, data), data, seed=9)
        IG.configure(smp, stree, [SP8]*6, "uniform", theta_prior=(2.0, 1000.0, 0.001), tau_prior=(3.0, 3.0/stree[1][-1]), kinds=kinds)
        smp.initialize()
        smp.iterate(50)
        assert smp.kind() == "generic"
        runs.append(_state(smp, 6))
        smp.close()
    assert runs[0] == runs[1]
    assert runs[0] != runs[2]                                # (and the other family is another chain)
    eng.close()


@pytest.mark.parametrize("which,moves", [("generic", "uniform"), ("generic", "program"), ("big", "uniform"), ("big", "program")])
def test_state_invariants_after_inverse_gamma_runs(which, moves):
    """100 iterations under inverse-gamma priors, then tests/invariants.py's recompute of every locus's likelihood, density,
    populations and buffers from (tree, taus, thetas)"""
    stree = synth.species_tree_arrays(4)
    data = gtr8(6)
    eng = bpp_amd.Engine(0)
    loci = tape.make_engine_loci(eng, data)
    smp = bpp_amd.Sampler(eng, loci, data, seed=19, implementation="big" if which == "big" else None)
    program = moves == "program"
    IG.configure(smp, stree, [SP8]*6, moves, theta_prior=(3.0, 0.004, 0.0004 if program else 0.001),
                 finetune=(0.003, 0.005, 0.0004, 0.05) if program else (0.003, 0.005, 0.0008, 0.2))
    smp.initialize()
    assert smp.kind() == which
    smp.iterate(100)
    seen = invariants.check_state(smp, data, stree[0], tip_species=[SP8]*6, loci=loci)
    print(which, moves, seen)
    moved(smp, stree)
    smp.close(); eng.close()
