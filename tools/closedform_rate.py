"""iterations/s and launches per iteration of the generic sampler on a strong-scaling rank's share of config 3's shape (1 250
loci x 8 taxa x 1 000 sites, four rate categories) simulated under HKY: the loci declared HKY (3 + 1 + 1 parameter steps) against
the same alignments declared GTR (3 + 5 + 1).  The models differ: a cost comparison, not an equality.
usage: python tools/closedform_rate.py [loci] [iterations] [hky|gtr|both]     (one MI355X)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bpp_amd
from bpp_amd import synth

NLOCI = int(sys.argv[1]) if len(sys.argv) > 1 else 1250
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 300
WHICH = sys.argv[3] if len(sys.argv) > 3 else "both"
MODEL = {"hky": bpp_amd.MODEL_HKY, "gtr": bpp_amd.MODEL_GTR}


def loci_for(eng, data, model):
    out = []
    for d in data:
        tips, sites = len(d["seqs"]), len(d["seqs"][0])
        loc = bpp_amd.Locus(eng, bpp_amd.DATA_DNA, MODEL[model], tips, 2*(tips - 1), 4, sites, 1, 2*(2*tips - 2), d["rate_cats"], 0)
        for i, s in enumerate(d["seqs"]):
            loc.set_tip_states(i, s)
        loc.set_pattern_weights(d["weights"])
        loc.set_frequencies(0, d["freqs"]); loc.set_subst_params(0, d["exch"]); loc.set_category_rates(d["rates"])
        out.append(loc)
    return out


data = synth.make_dataset(NLOCI, 1000, 8, "hky", 4, seed=12345, kappa=3.0)
eng = bpp_amd.Engine(0)
for model in (("hky", "gtr", "hky", "gtr") if WHICH == "both" else (WHICH,)):
    smp = bpp_amd.Sampler(eng, loci_for(eng, data, model), data, seed=3)
    smp.set_proposal_kernel(1); smp.set_program_moves(True, 0.1)             # bench.py's set-up of config 3
    par, tau, theta = synth.species_tree_arrays(8)
    smp.set_species_tree(par, tau, theta)
    smp.set_tau_prior(3.0, 3.0/tau[-1]); smp.set_theta_prior(2.0, 2.0/theta[0], 0.001); smp.set_finetune(5.0, 0.001, 0.001, 0.3)
    for i, d in enumerate(data):
        smp.set_subst_model(i, d["freqs"], d["exch"], 0.5)
    smp.set_subst_moves(0.2, 0.3, 0.5, 1.0, 1.0)
    smp.set_qrates_prior((2, 4, 2, 2, 4, 2))
    smp.initialize()
    smp.burnin(100); smp.iterate(20); eng.synchronize()
    l0 = smp.summary()["launches"]
    smp.enable_timing(7)
    t0 = time.perf_counter(); smp.iterate(ITERS); eng.synchronize(); dt = time.perf_counter() - t0
    tm = smp.timing()
    l1 = smp.summary()["launches"]
    print(f"{NLOCI} loci declared {model}: steps {smp.subst_steps()}, {ITERS/dt:8.1f} it/s, {dt/ITERS*1e3:.3f} ms/iteration, "
          f"{(l1 - l0)/ITERS:.1f} launches/iteration (timed launches, every 7th: per-locus {tm['sweep_launches']}, all-loci {tm['allloci_launches']})", flush=True)
    smp.close()
eng.close()
