"""The big-tree sampler's rate under both move sets on ONE build: the frogs loci (BASELINE config 1, set up as bench.py's
run_config1) and twelve 24-tip loci with scale buffers (the set of tests/test_gpu_bigsampler.py), each with the library's own
uniform windows and with BPP's kernel + the program's moves (bpa_sampler_set_proposal_kernel / bpa_sampler_set_program_moves).

    python tools/big_moves_rate.py [--runs 3] [--rounds 1] [--yardstick DIR] [--subst]

`--subst` adds six 17-tip GTR+Gamma4 loci, under each move set without and with the three substitution-parameter moves
(bpa_sampler_set_subst_moves: nine more steps of all loci an iteration) — keys `<moves>` and `<moves>_subst`.

One child process per case (a fresh device context each: no case inherits another's warmed state); a child warms up, then times
`--runs` windows of whole iterations, each ended by a device synchronise.  `--rounds N` walks the list of cases N times, so
that the cases alternate.  `--yardstick DIR`: another checkout of this repository WITH ITS LIBRARY BUILT (the parent commit,
say) — its uniform-window rates are measured by the same children in the same walk; that tree refuses BPP's kernel on big
trees, so only its uniform cases run.  Output: one JSON line (iterations/s per window, their min and max).
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = {"frogs": 40, "tips24": 150}                   # timed iterations per window (~1 s of launches each)
SUBST_DATA = {"gtr17": 150}                           # --subst: six 17-tip GTR+Gamma4 loci of about 30 patterns (shapes.shaped_set)


def child(root, data_name, moves, runs, iters, subst=False):
    sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
    import numpy as np
    import bpp_amd
    from bpp_amd import seqio, synth
    import tape
    eng = bpp_amd.Engine(0)
    if data_name == "frogs":
        g = os.path.join(root, "tests", "golden", "frogs")
        recs = seqio.load_dataset(os.path.join(g, "frogs.txt"), os.path.join(g, "frogs.Imap.txt"), ["K", "C", "L", "H"], [1, 1, 1, 1], model="jc69")
        parent, tau0, thetas = [4, 4, 5, 6, 5, 6, -1], [0.0] * 4 + [0.01, 0.02, 0.03], [0.02] * 7
        rng = np.random.default_rng(9)
        data = []
        for r in recs:
            left, right, times, root_ = synth.msc_start_tree(r["species"], parent, tau0, thetas, rng)
            data.append(dict(seqs=r["seqs"], weights=r.get("weights", np.ones(len(r["seqs"][0]))), left=left, right=right, times=times,
                             root=root_, states=4, rate_cats=1, model="jc69", rates=np.ones(1)))
        species = [r["species"] for r in recs]
        loci = [seqio.make_locus(eng, r) for r in recs]
        tau_prior, theta_prior, ft = (3.0, 100.0), (3.0, 150.0, 0.003), (0.004, 0.004, 0.002, 0.1)
    elif data_name == "gtr17":
        import shapes
        parent, tau0, thetas = stree = synth.species_tree_arrays(8)
        sp = [0, 0, 0] + [k // 2 for k in range(2, 16)]
        data = shapes.shaped_set(sp, stree, [28 + k % 5 for k in range(6)], 90, model="gtr", rate_cats=4)
        species = [sp] * len(data)
        loci = tape.make_engine_loci(eng, data)
        tau_prior, theta_prior, ft = (3.0, 3.0 / tau0[-1]), (2.0, 1000.0, 0.0004 if moves == "program" else 0.001), (0.003, 0.005, 0.0004, 0.05)
    else:
        rng = np.random.default_rng(5)
        parent, tau0, thetas = synth.species_tree_arrays(4, 0.004)
        sp = [k // 6 for k in range(24)]
        data = []
        for _ in range(12):
            left, right, times, root_ = synth.msc_start_tree(sp, parent, tau0, thetas, rng)
            base = "".join(rng.choice(list("ACGT"), 200))
            seqs = ["".join(c if rng.random() > 0.04 else rng.choice(list("ACGT")) for c in base) for _ in range(24)]
            pats, w = bpp_amd.compress_site_patterns(seqs, True, True)
            data.append(dict(seqs=pats, weights=w, left=left, right=right, times=times, root=root_, states=4, rate_cats=1, model="jc69", rates=np.ones(1)))
        species = [sp] * len(data)
        loci = tape.make_engine_loci(eng, data, True)
        tau_prior, theta_prior, ft = (3.0, 3.0 / tau0[-1]), (2.0, 500.0, 0.001), (0.002, 0.003, 0.0004, 0.1)
    smp = bpp_amd.Sampler(eng, loci, data, seed=1)
    if moves == "program":
        smp.set_proposal_kernel(1)
        smp.set_program_moves(True, 0.1)
    smp.set_species_tree(parent, tau0, thetas)
    for i in range(len(data)):
        smp.set_tip_species(i, species[i])
    smp.set_tau_prior(*tau_prior)
    smp.set_theta_prior(*theta_prior)
    smp.set_finetune(*ft)
    if subst:
        # the three substitution-parameter moves (nine steps of all loci an iteration), locusrates.configure's widths and prior
        for i, d in enumerate(data):
            smp.set_subst_model(i, d["freqs"], d["exch"], 0.5)
        smp.set_subst_moves(0.3, 0.4, 0.8, 1.0, 1.0)
    smp.initialize()
    assert smp.kind() == "big", smp.kind()
    smp.iterate(5)
    eng.synchronize()
    l0 = smp.summary()["launches"]
    rates = []
    for _ in range(runs):
        t0 = time.perf_counter()
        smp.iterate(iters)
        eng.synchronize()
        rates.append(iters / (time.perf_counter() - t0))
    sm = smp.summary()
    print(json.dumps(dict(rates=[round(x, 2) for x in rates], iterations=iters, loci=len(data),
                          launches_per_iteration=round((sm["launches"] - l0 - 1) / (runs * iters), 1),
                          acceptance=round(sm["accepted"] / max(sm["proposals"], 1), 3))), flush=True)
    smp.close(); eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--yardstick", default=None)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--child", nargs=3, metavar=("ROOT", "DATA", "MOVES"), default=None)
    ap.add_argument("--iters", type=int, default=0)
    ap.add_argument("--subst", action="store_true", help="also the 17-tip GTR+Gamma4 set, each move set without and with the three substitution-parameter moves")
    ap.add_argument("--subst-on", action="store_true", help="(child) switch the three moves on")
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.child[2], a.runs, a.iters or {**DATA, **SUBST_DATA}[a.child[1]], a.subst_on)
    cases = [("this", HERE, d, m) for d in DATA for m in ("uniform", "program")]
    if a.yardstick:
        cases += [("yardstick", os.path.abspath(a.yardstick), d, "uniform") for d in DATA]
    cases.sort(key=lambda c: (c[2], c[0] != "yardstick", c[3]))                  # per data set: yardstick, uniform, program
    if a.subst:
        cases += [(who, HERE, d, m) for d in SUBST_DATA for m in ("uniform", "program") for who in ("this", "subst")]
    out = {}
    for _ in range(a.rounds):
        for who, root, d, m in cases:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", root, d, m, "--runs", str(a.runs)] + (["--iters", str(a.iters)] if a.iters else []) + \
                  (["--subst-on"] if who == "subst" else [])
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
                rc, err = r.returncode, r.stderr
            except subprocess.TimeoutExpired as ex:
                rc, err = f"none within {a.timeout} s", (ex.stderr.decode(errors="replace") if isinstance(ex.stderr, bytes) else ex.stderr or "")
            if rc != 0:
                # a child that died or hung may have left the device in a bad way: nothing more is started on it
                print(json.dumps(dict(error=f"{who} {d} {m}: exit {rc}", stderr=err[-1500:], partial=out)), flush=True)
                return 1
            res = json.loads(r.stdout.strip().splitlines()[-1])
            e = out.setdefault(d, {}).setdefault(m if who == "this" else m + "_subst" if who == "subst" else "yardstick_uniform", dict(rates=[]))
            e["rates"] += res.pop("rates")
            e.update(res)
    for d in out.values():
        for e in d.values():
            e["min"], e["max"] = min(e["rates"]), max(e["rates"])
    print(json.dumps(dict(tool="big_moves_rate", unit="iterations/s", runs_per_child=a.runs, rounds=a.rounds, **out)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
