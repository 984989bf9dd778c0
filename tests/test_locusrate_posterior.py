"""End-to-end known answer for the per-locus mutation rates (mu_i, mu_bar: prop_locusrate_mui stree.c:9225,
prop_locusrate_mubar stree.c:9770): the posterior of the UNMODIFIED reference program with `locusrate = 1 10 10 5 iid` on a
synthetic 20-locus 4-species JC69 data set (fixture tests/golden/locusrate_posterior.json from
tests/golden/make_golden_locusrate.py: thetaprior gamma 2 500, tauprior gamma 2 300; the program's seed 2 lies within these
bars of its seed 1, which is the fixture) against this repo's samplers on the same data and priors — every theta, every tau,
mu_bar and the log-likelihood within tests/test_gtr_posterior.py's bars (0.3 sd on the means, 0.25 sd on the sds).

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
import locusrates as LR

HERE = os.path.dirname(os.path.abspath(__file__))
POP_OF = {"A,B": 4, "A,B,C": 5, "A,B,C,D": 6}           # synth.species_tree_arrays(4): tips, then children before parents


@pytest.fixture(scope="module")
def gold():
    return json.load(open(os.path.join(HERE, "golden", "locusrate_posterior.json")))


def dataset(gold):
    c = gold["config"]
    return synth.make_dataset(c["nloci"], c["sites"], c["taxa"], "jc69", 1, seed=c["seed"], theta=c["theta"])


def setup(drv, gold, program=False):
    c = gold["config"]
    parent, tau, thetas = synth.species_tree_arrays(c["taxa"], c["theta"])
    drv.set_species_tree(parent, tau, thetas)
    drv.set_tau_prior(*c["tau_prior"])
    # step lengths for acceptance rates of 0.2 - 0.5 (measured on the host driver: tree moves and all-loci steps 0.50 pooled, MUI
    # 0.34, MUBAR 0.20).  mu_bar and the taus lie on a ridge (the data fix their product): the slowest direction of this chain
    # (BPP's Bactrian-Laplace variate has unit variance, a uniform window of width 1 a standard deviation of 0.29: the program's
    # moves take shorter step lengths for the same rates — measured there: 0.34 pooled, MUI 0.35, MUBAR 0.21)
    drv.set_theta_prior(c["theta_prior"][0], c["theta_prior"][1], 0.004 if program else 0.008)
    if program:
        drv.set_finetune(0.004, 0.004, 0.0012, 0.2)
    else:
        drv.set_finetune(0.006, 0.006, 0.003, 0.8)
    a_mubar, b_mubar, a_mui = c["locusrate"]
    # BPP's start: every rate and the mean at 1
    drv.set_locusrate_moves(0.6 if program else 2.5, 0.3 if program else 1.5, a_mui, a_mubar, b_mubar, 1.0)


def sample(drv, host):
    mubar = drv.get_locus_rates()[1]
    lnl = drv.total_lnl() if host else drv.summary()["total_lnl"]
    return list(drv.thetas()[4:]) + list(drv.taus()[4:]) + [mubar, lnl]


def compare(samples, gold):
    """tests/test_gtr_posterior.py's compare with this fixture's columns: thetas[4..6], taus[4..6], mu_bar, lnL"""
    c = gold["config"]
    S = np.array(samples)
    seen = set()
    for name, ref in gold["posterior"].items():
        if name == "lnL":
            x = S[:, 7]
        elif name == "mu_bar":
            x = S[:, 6]
        else:
            kind, _, label = name.split(":")
            x = S[:, POP_OF[label] - 4 + (0 if kind == "theta" else 3)]
        seen.add(name)
        print(f"{name}: mean {x.mean():.6g} (program {ref['mean']:.6g}, {abs(x.mean() - ref['mean'])/ref['sd']:.3f} sd), sd {x.std():.6g} (program {ref['sd']:.6g})")
        assert abs(x.mean() - ref["mean"]) < c["tol_mean"]*ref["sd"], (name, x.mean(), ref["mean"], ref["sd"])
        assert abs(x.std() - ref["sd"]) < c["tol_sd"]*ref["sd"], (name, x.std(), ref["sd"])
    assert len(seen) == 8 and "mu_bar" in seen and (c["tol_mean"], c["tol_sd"]) == (0.3, 0.25)


@pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref not built")
def test_host_driver_with_rate_moves_reproduces_bpp_posterior(gold):
    data = dataset(gold)
    drv = LR.reference_driver(data, seed=5)
    setup(drv, gold)
    drv.initialize()
    S = []
    for it in range(9000):
        drv.iterate()
        if it >= 2000 and it % 2 == 0:
            S.append(sample(drv, True))
    compare(S, gold)
    c = drv.locusrate_counters()
    assert 0.1 < c["mui"][1]/c["mui"][0] < 0.9 and 0.1 < c["mubar"][1]/c["mubar"][0] < 0.9
    drv.close()


# 2 000 + 8 000 iterations, thinned by 2: 3.1 s (uniform) and 3.8 s (the program's moves) on an MI355X, so not halved.  At this length the Monte-Carlo error of the slowest quantity (mu_bar's mean) is
# 0.02 - 0.28 sd over the seeds tried on the CPU twin (the host driver, which the uniform leg follows decision by decision:
# seeds 9, 10, 12 -> worst mean 0.28, 0.14, 0.13 sd; worst sd 0.14, 0.12, 0.10) against the bar of 0.3: the seed is fixed at 10.
# The program's moves at their step lengths, same twin: seeds 9, 10, 13 -> worst mean 0.08, 0.06, 0.22 sd.
@pytest.mark.gpu
@pytest.mark.parametrize("moves", ["uniform", "program"])
def test_device_sampler_with_rate_moves_reproduces_bpp_posterior(gold, moves):
    import bpp_amd
    import tape
    data = dataset(gold)
    eng = bpp_amd.Engine(0)
    dev = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, data), data, seed=10, implementation="generic")
    if moves == "program":
        dev.set_proposal_kernel(1)
        dev.set_program_moves(True, 0.1)
    setup(dev, gold, moves == "program")
    dev.initialize()
    assert dev.kind() == "generic"
    dev.iterate(2000)
    S = []
    for _ in range(4000):
        dev.iterate(2)
        S.append(sample(dev, False))
    compare(S, gold)
    c = dev.locusrate_counters()
    assert 0.1 < c["mui"][1]/c["mui"][0] < 0.9 and 0.1 < c["mubar"][1]/c["mubar"][0] < 0.9
    dev.close(); eng.close()
