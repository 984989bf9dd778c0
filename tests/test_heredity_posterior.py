"""End-to-end known answer for the heredity scalars (gtree_update_logprob_contrib gtree.c:3859, prop_heredity gtree.c:8214):
the posterior of the UNMODIFIED reference program on a synthetic 20-locus 4-species JC69 data set in both forms of the control
file's `heredity` line — `heredity = 1 4 4` (estimated, h_i ~ gamma(4, 4)) and `heredity = 2 file` (fixed, the loci cycling
through 1.0 / 0.75 / 0.25) — (fixture tests/golden/heredity_posterior.json from tests/golden/make_golden_heredity.py:
thetaprior gamma 2 500, tauprior gamma 2 300; the program's seed 2 lies within these bars of its seed 1, which is the fixture)
against this repo's samplers on the same data and priors: every theta, every tau and the log-likelihood within
tests/test_gtr_posterior.py's bars (0.3 sd on the means, 0.25 sd on the sds).  The two forms' posteriors are far apart (the
root's theta: 0.0045 against 0.0062, its sd 0.0014), and both from the posterior without scalars.

 * CPU: the C host driver on the REAL reference's locus API (skipped where oracle/_ref is absent);
 * GPU: the generic device-resident sampler (implementation="generic": these loci would fit the LDS kernels) with the uniform kernel
   and with the program's moves.
"""
import json
import os

import numpy as np
import pytest

from bpp_amd import synth
import oraclelib as O
import heredity as HD

HERE = os.path.dirname(os.path.abspath(__file__))
POP_OF = {"A,B": 4, "A,B,C": 5, "A,B,C,D": 6}           # synth.species_tree_arrays(4): tips, then children before parents


@pytest.fixture(scope="module")
def gold():
    return json.load(open(os.path.join(HERE, "golden", "heredity_posterior.json")))


def dataset(gold):
    c = gold["config"]
    return synth.make_dataset(c["nloci"], c["sites"], c["taxa"], "jc69", 1, seed=c["seed"], theta=c["theta"])


def setup(drv, gold, form, program=False):
    c = gold["config"]
    parent, tau, thetas = synth.species_tree_arrays(c["taxa"], c["theta"])
    drv.set_species_tree(parent, tau, thetas)
    drv.set_tau_prior(*c["tau_prior"])
    # the step lengths of tests/test_locusrate_posterior.py (same data, same priors)
    drv.set_theta_prior(c["theta_prior"][0], c["theta_prior"][1], 0.004 if program else 0.008)
    if program:
        drv.set_finetune(0.004, 0.004, 0.0012, 0.2)
    else:
        drv.set_finetune(0.006, 0.006, 0.003, 0.8)
    if form == "estimated":
        # (BPP starts at a/b (0.8 + 0.4 u); here: the prior mean)
        drv.set_heredity(np.full(c["nloci"], c["heredity_prior"][0]/c["heredity_prior"][1]))
        drv.set_heredity_move(0.8 if program else 2.5, *c["heredity_prior"])
    else:
        drv.set_heredity([c["heredity_fixed"][i % 3] for i in range(c["nloci"])])


def sample(drv, host):
    lnl = drv.total_lnl() if host else drv.summary()["total_lnl"]
    return list(drv.thetas()[4:]) + list(drv.taus()[4:]) + [lnl]


def compare(samples, gold, form):
    c = gold["config"]
    S = np.array(samples)
    seen = set()
    for name, ref in gold[form]["posterior"].items():
        if name == "lnL":
            x = S[:, 6]
        else:
            kind, _, label = name.split(":")
            x = S[:, POP_OF[label] - 4 + (0 if kind == "theta" else 3)]
        seen.add(name)
        print(f"{form} {name}: mean {x.mean():.6g} (program {ref['mean']:.6g}, {abs(x.mean() - ref['mean'])/ref['sd']:.3f} sd), sd {x.std():.6g} (program {ref['sd']:.6g}, {abs(x.std() - ref['sd'])/ref['sd']:.3f})")
        assert abs(x.mean() - ref["mean"]) < c["tol_mean"]*ref["sd"], (name, x.mean(), ref["mean"], ref["sd"])
        assert abs(x.std() - ref["sd"]) < c["tol_sd"]*ref["sd"], (name, x.std(), ref["sd"])
    assert len(seen) == 7 and (c["tol_mean"], c["tol_sd"]) == (0.3, 0.25)


def check_counters(drv, form, iters, n):
    p, a = drv.heredity_counters()
    if form == "estimated":
        assert p == iters*n and 0.1 < a/p < 0.9, (p, a)
    else:
        assert (p, a) == (0, 0)
        assert list(drv.get_heredity()[:3]) == [1.0, 0.75, 0.25]


@pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("form", ["estimated", "fixed"])
def test_host_driver_with_heredity_reproduces_bpp_posterior(gold, form):
    data = dataset(gold)
    drv = HD.reference_driver(data, seed=5)
    setup(drv, gold, form)
    drv.initialize()
    S = []
    for it in range(9000):
        drv.iterate()
        if it >= 2000 and it % 2 == 0:
            S.append(sample(drv, True))
    compare(S, gold, form)
    check_counters(drv, form, 9000, len(data))
    drv.close()


# 2 000 + 8 000 iterations thinned by 2, as tests/test_locusrate_posterior.py's device legs
@pytest.mark.gpu
@pytest.mark.parametrize("moves", ["uniform", "program"])
@pytest.mark.parametrize("form", ["estimated", "fixed"])
def test_device_sampler_with_heredity_reproduces_bpp_posterior(gold, form, moves):
    import bpp_amd
    import tape
    data = dataset(gold)
    eng = bpp_amd.Engine(0)
    dev = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, data), data, seed=10, implementation="generic")
    if moves == "program":
        dev.set_proposal_kernel(1)
        dev.set_program_moves(True, 0.1)
    setup(dev, gold, form, moves == "program")
    dev.initialize()
    assert dev.kind() == "generic"
    dev.iterate(2000)
    S = []
    for _ in range(4000):
        dev.iterate(2)
        S.append(sample(dev, False))
    compare(S, gold, form)
    check_counters(dev, form, 10000, len(data))
    dev.close(); eng.close()
