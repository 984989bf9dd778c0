"""The yardstick of tests/test_gpu_bigsampler_scalars.py, on the CPU: the C host driver on the REAL reference's locus API with
HRDT, MUI and MUBAR on together, on loci of the big-tree sampler's kind (17 tips; 24 tips whose scale counters fire), leaves
a state that is its CPU recompute at (tree, taus, thetas, h_i, lengths x mu_i) — and the rates the firing test sets keep the
oracle's counters firing at the start trees."""
import numpy as np
import pytest

import firing
import heredity as HD
import hostdrv
import locusrates as LR
import oraclelib as O
import shapes
from test_gpu_bigsampler_scalars import FIRING_RATES, HRDT, RATE_FT, A_MUI, MUBAR_PRIOR, _rated_firing

needs_ref = pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref not built")


def test_the_firing_rates_keep_the_counters_firing_at_the_start():
    """firing.fires_at_start's conditions on the oracle at the start trees' lengths x mu_i, and rates that differ"""
    data = firing.case("big-24")["data"]
    mui = LR.spread_rates(len(data), *FIRING_RATES)
    assert mui.min() == FIRING_RATES[0] and mui.max() == FIRING_RATES[1]
    with _rated_firing(data, mui) as tagged:
        firing.fires_at_start(tagged)
        rated = firing.summary(tagged)
    print(f"nodes with a counter / largest counter per locus: unscaled {firing.summary(data)}, at lengths x mu_i {rated}")


@needs_ref
@pytest.mark.parametrize("name,moves", [("big-17-30", "uniform"), ("big-17-30", "program"), ("big-24", "uniform"), ("big-24", "program")])
def test_host_driver_state_with_all_three_moves(name, moves):
    """20 iterations; every locus's density the one-locus driver's at h_i (1e-11), its lnl the oracle's at lengths x mu_i
    (1e-12), tree shape, populations and buffer indices sound (heredity.check_state, rated); every move proposed and moved"""
    fires = name == "big-24"
    c = firing.case(name) if fires else shapes.case(name)
    data, n = c["data"], len(c["data"])
    drv = HD.reference_driver(data, seed=31) if not fires else HD.HeredDriver(hostdrv.reference_driver(data, seed=31, scaling=True))
    shapes.configure(drv, c, moves, host=True)
    rates = LR.spread_rates(n, *(FIRING_RATES if fires else (0.5, 2.0)))
    h0 = HD.start_scalars(n)
    drv.set_locus_rates(rates)
    # (the firing set: the narrow rate prior and window of the GPU test, so that the chain stays where the counters fire)
    if fires:
        drv.set_locusrate_moves(0.05, 0.05, 200.0, MUBAR_PRIOR[0], MUBAR_PRIOR[1], 1.0)
    else:
        drv.set_locusrate_moves(RATE_FT[0], RATE_FT[1], A_MUI, MUBAR_PRIOR[0], MUBAR_PRIOR[1], 1.0)
    drv.set_heredity(h0)
    drv.set_heredity_move(*HRDT)
    drv.initialize()
    HD.check_state(drv, data, c["stree"][0], rated=True, scaling=fires, tip_species=c["species"])
    for _ in range(20):
        drv.iterate()
    seen = HD.check_state(drv, data, c["stree"][0], rated=True, scaling=fires, tip_species=c["species"])
    hp, ha = drv.heredity_counters()
    cnt = drv.locusrate_counters()
    print(f"{name} {moves}: {seen}; HRDT {ha}/{hp}, MUI {cnt['mui']}, MUBAR {cnt['mubar']}")
    assert hp == 20*n and 0 < ha < hp
    assert cnt["mui"][0] == 20*n and 0 < cnt["mui"][1] < 20*n and cnt["mubar"][0] == 20
    mui, mubar = drv.get_locus_rates()
    assert (mui != rates).any() and (drv.get_heredity() != h0).any()
    if fires:
        with _rated_firing(data, mui) as tagged:
            firing.still_fires(tagged, [drv.tree(i) for i in range(n)])
    drv.close()
