"""iterations/s of the generic device sampler around the heredity scalars (NOTES: the section on the heredity scalars).

    python tools/heredity_rates.py existing     config 3 (10 000 GTR+G4 loci) and config 5 (anopheles), heredity never set
    python tools/heredity_rates.py cost         200 GTR+G4 8-tip loci of ~30 patterns and 1 250 config-3 loci: nothing set /
                                                fixed scalars / HRDT on

BPP_AMD_TREE=<dir>: import bpp_amd from there (another build's package + libraries) — `existing` on two builds in one call is how
the equal-within-spread check is made.  One JSON line per measurement."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("BPP_AMD_TREE", ROOT)); sys.path.insert(1, os.path.join(ROOT, "tests")); sys.path.insert(2, ROOT)
import numpy as np
import bpp_amd
from bpp_amd import synth
import tape


def rate(smp, eng, warm, iters):
    smp.initialize(); smp.iterate(warm); eng.synchronize()
    l0 = smp.summary()["launches"]; eng.synchronize()
    t0 = time.perf_counter(); smp.iterate(iters); eng.synchronize(); dt = time.perf_counter() - t0
    return dict(iterations_per_s=round(iters/dt, 2), launches_per_iteration=round((smp.summary()["launches"] - l0 - 1)/iters, 1), kind=smp.kind())


def gtr_sampler(eng, data, taxa, hered):
    """hered: None nothing set, 'fixed' scalars cycling 1 / 0.75 / 0.25, 'move' the same start with HRDT on"""
    smp = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, data), data, seed=3)
    par, tau, theta = synth.species_tree_arrays(taxa)
    smp.set_species_tree(par, tau, theta)
    smp.set_tau_prior(3.0, 3.0/tau[-1]); smp.set_theta_prior(2.0, 1000.0, 0.001)
    smp.set_finetune(0.003, 0.005, 0.0008, 0.2)
    smp.set_subst_moves(0.3, 0.4, 0.8, 1.0, 1.0)
    for i, d in enumerate(data):
        smp.set_subst_model(i, d["freqs"], d["exch"], 0.5)
    if hered:
        smp.set_heredity([(1.0, 0.75, 0.25)[i % 3] for i in range(len(data))])
        if hered == "move":
            smp.set_heredity_move(0.6, 4.0, 4.0)
    return smp


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "cost"
    eng = bpp_amd.Engine(0)
    tree = os.environ.get("BPP_AMD_TREE", "this tree")
    if what == "existing":
        data = synth.make_dataset(10000, 1000, 8, "gtr", 4, seed=12345)
        for rep in range(2):
            smp = gtr_sampler(eng, data, 8, None)
            print(json.dumps(dict(what="config 3, 10 000 loci, heredity never set", tree=tree, rep=rep, **rate(smp, eng, 20, 150))), flush=True)
            smp.close()
        import importlib.util
        spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py")); b = importlib.util.module_from_spec(spec); spec.loader.exec_module(b)
        for rep in range(2):
            r = b.run_config5(eng, 400)
            print(json.dumps(dict(what="config 5 (bench.py run_config5, 400 iterations)", tree=tree, rep=rep, iterations_per_s=r["iterations_per_s"], launches_per_iteration=r["launches_per_iteration"])), flush=True)
    else:
        import locusrates as LR
        sets = [("200 GTR+G4 8-tip loci of ~30 patterns", LR.case("b")["data"], 300, 2000), ("1 250 config-3 loci", synth.make_dataset(1250, 1000, 8, "gtr", 4, seed=12345), 100, 600)]
        for name, data, warm, iters in sets:
            for hered in (None, "fixed", "move", None, "fixed", "move"):
                smp = gtr_sampler(eng, data, 8, hered)
                print(json.dumps(dict(what=name, heredity=hered or "never set", **rate(smp, eng, warm, iters))), flush=True)
                smp.close()
    eng.close()


if __name__ == "__main__":
    main()
