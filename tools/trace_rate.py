"""What a posterior sample costs: the sample trace (bpa_sampler_set_trace) against stopping the chain to look, on config 2's
shape (10 000 four-tip JC69 loci, the program's moves on the persistent kernel, after the bench's burn-in) and config 3's
(10 000 eight-tip GTR+Gamma4 loci, the program's moves on the generic sampler).

    python tools/trace_rate.py [--shapes c2,c3] [--loci 10000] [--repeats 3] [--window 1.0] [--parent DIR]

Figures, iterations/s, each over a window of at least `--window` seconds after warm-up, `--repeats` times, the variants
taking turns inside one process on ONE sampler (so every variant meets the same device state and the same chain):
  a        untraced iterate(N), one synchronise at the end of the window
  b[k]     traced with every = k in 1, 2, 10, 100: iterate(N), then trace_read() of the whole window's rows (inside the window)
  c[k]     stop and look: iterate(k), taus(), thetas(), summary() in a loop
  d        `--parent DIR`: (a) on another checkout of this repository WITH ITS LIBRARY BUILT (the parent commit), by a child
           process of its own before and after this tree's child — the same code path, so it differs from (a) by the spread only
row_cost_us[k] = (1/median b[k] - 1/median a) k: what one row boundary adds.  Output: one JSON object.
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVERY = (1, 2, 10, 100)


def child(root, shape, nloci, repeats, window, only_a):
    sys.path.insert(0, HERE)            # bench.py (the configurations, the loci, the program's step lengths)
    sys.path.insert(0, root)            # ... and the library under test
    import bench
    import bpp_amd
    from bpp_amd import synth
    cfg = bench.CONFIGS[shape]
    data = synth.make_dataset(nloci, cfg["sites"], cfg["taxa"], cfg["model"], cfg["rate_cats"], seed=12345)
    eng = bpp_amd.Engine(0)
    smp = bpp_amd.Sampler(eng, bench.make_loci(eng, data), data, seed=1)
    parent, tau, theta = synth.species_tree_arrays(cfg["taxa"])
    smp.set_proposal_kernel(1)
    smp.set_program_moves(True, 0.1)
    smp.set_species_tree(parent, tau, theta)
    smp.set_tau_prior(3.0, 3.0 / tau[-1])
    if cfg["model"] == "jc69":          # bench.run_sampler's settings for the headline
        scale = math.sqrt(10000.0 / nloci)
        smp.set_theta_prior(2.0, 2.0 / theta[0], bench.PROGRAM_FT["theta"] * scale)
        smp.set_finetune(bench.PROGRAM_FT["gage"], bench.PROGRAM_FT["gspr"], bench.PROGRAM_FT["tau"] * scale, bench.PROGRAM_FT["mix"] * scale)
    else:
        smp.set_theta_prior(2.0, 2.0 / theta[0], 0.001)
        smp.set_finetune(5.0, 0.001, 0.001, 0.3)
        for i, d in enumerate(data):
            smp.set_subst_model(i, d["freqs"], d["exch"], 0.5)
        smp.set_subst_moves(0.2, 0.3, 0.5, 1.0, 1.0)
    smp.initialize()
    kind = smp.kind()
    smp.burnin(800 if cfg["model"] == "jc69" else 400)
    smp.iterate(20)
    eng.synchronize()
    t0 = time.perf_counter()
    probe = 200 if cfg["model"] == "jc69" else 10
    smp.iterate(probe)
    eng.synchronize()
    n = max(100, int(math.ceil(1.15 * window * probe / (time.perf_counter() - t0) / 100.0)) * 100)      # a multiple of every k

    def run_a():
        t = time.perf_counter()
        smp.iterate(n)
        eng.synchronize()
        return n / (time.perf_counter() - t)

    def run_b(k):
        smp.set_trace(k, 4096)
        t = time.perf_counter()
        smp.iterate(n)
        rows = smp.trace_read()
        dt = time.perf_counter() - t
        assert len(rows) == n // k, (len(rows), n, k)
        smp.set_trace(0, 0)
        return n / dt

    def run_c(k):
        done, t = 0, time.perf_counter()
        while True:
            smp.iterate(k)
            smp.taus(); smp.thetas(); smp.summary()
            done += k
            dt = time.perf_counter() - t
            if dt >= window:
                return done / dt

    out = dict(kind=kind, loci=nloci, iterations_per_window=n, a=[])
    if not only_a:
        out["b"] = {k: [] for k in EVERY}
        out["c"] = {k: [] for k in EVERY}
    for _ in range(repeats):
        out["a"].append(run_a())
        if only_a:
            continue
        for k in EVERY:
            out["b"][k].append(run_b(k))
            out["c"][k].append(run_c(k))
    print(json.dumps(out), flush=True)
    smp.close(); eng.close()


def spread(v):
    return dict(rates=[round(x, 2) for x in v], min=round(min(v), 2), median=round(statistics.median(v), 2), max=round(max(v), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c3")
    ap.add_argument("--loci", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--timeout", type=int, default=420, help="seconds per child")
    ap.add_argument("--child", nargs=2, metavar=("ROOT", "SHAPE"), default=None)
    ap.add_argument("--only-a", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.loci, a.repeats, a.window, a.only_a)
    res = dict(tool="trace_rate", unit="iterations/s", window_s=a.window, repeats=a.repeats)
    for shape in a.shapes.split(","):
        runs = [("this", HERE)]
        if a.parent:
            runs = [("parent", os.path.abspath(a.parent))] + runs + [("parent", os.path.abspath(a.parent))]
        got = {}
        for who, root in runs:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", root, shape, "--loci", str(a.loci), "--repeats", str(a.repeats),
                   "--window", str(a.window)] + (["--only-a"] if who == "parent" else [])
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
                rc, err = r.returncode, r.stderr
            except subprocess.TimeoutExpired as ex:
                rc, err = f"none within {a.timeout} s", (ex.stderr.decode(errors="replace") if isinstance(ex.stderr, bytes) else ex.stderr or "")
            if rc != 0:
                # a child that died or hung may have left the device in a bad way: nothing more is started on it
                print(json.dumps(dict(error=f"{who} {shape}: exit {rc}", stderr=err[-1500:], partial=res)), flush=True)
                return 1
            o = json.loads(r.stdout.strip().splitlines()[-1])
            print(f"[trace_rate] {shape} {who}: a = {[round(x, 1) for x in o['a']]}", file=sys.stderr, flush=True)
            if who == "parent":
                got.setdefault("d", []).extend(o["a"])
            else:
                got.update(o)
        e = dict(kind=got["kind"], loci=got["loci"], iterations_per_window=got["iterations_per_window"], a=spread(got["a"]),
                 b={k: spread(v) for k, v in got["b"].items()}, c={k: spread(v) for k, v in got["c"].items()})
        if "d" in got:
            e["d"] = spread(got["d"])
        e["row_cost_us"] = {k: round((1.0 / e["b"][k]["median"] - 1.0 / e["a"]["median"]) * int(k) * 1e6, 2) for k in e["b"]}
        # (medians; where the two are within each other's spread — every = 100 on the slow shape: three rows a window — the
        #  rates printed above say so)
        e["b_not_below_c"] = {k: e["b"][k]["median"] >= e["c"][k]["median"] for k in e["b"]}
        res[shape] = e
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
