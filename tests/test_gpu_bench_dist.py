"""bench.py's N > 1 path end to end on the one-GPU test box: two ranks (gloo instead of RCCL, both on device 0) run the
sharded device-resident sampler (the headline) and the sharded tape with the per-step all-reduce of the partial sums —
under weak scaling (every rank its own data set) and strong scaling (ONE data set dealt out by the reference's zig-zag,
threads.c:265-353), over the default exchange (the framework's collective) and over the one-shot p2p exchange; the line
rank 0 prints must be the last line on stdout, carry the whole-job rate and pass its own all-reduce self-check."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(extra, tmp=None, world=2):
    """-> (the full record bench.py wrote to --full-record, stderr); the stdout line is the compact one the driver parses:
    checked here to be the last line, small, and to carry the contract's keys"""
    import tempfile
    full_path = os.path.join(tempfile.mkdtemp(prefix="bench_"), "full.json")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, BENCH_DIST_BACKEND="gloo", BENCH_FORCE_DEVICE="0")
    cmd = ([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
            "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--steps", "6", "--warmup", "2", "--full"] +
           ([] if "--loci" in extra else ["--loci", "1500"]) + ["--no-cpu-baseline", "--full-record", full_path] + extra)
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1]
    line = json.loads(last)
    assert len(last) <= 8192, len(last)
    full = json.load(open(full_path))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in line, k
    assert line["value"] == full["value"] and line["n_gpus"] == world and line["roofline"]["frac"] == full["roofline"]["frac"]
    assert line["value_weak"] == full["value_weak"] and line["value_strong"] == full["value_strong"]
    return full, r.stderr


@pytest.mark.parametrize("p2p,scaling", [(False, "weak"), (True, "weak"), (True, "strong")])      # (the default exchange with ONE data set: the test below)
def test_two_rank_bench_line(p2p, scaling):
    """p2p = False (--no-p2p, also what a failed mailbox self-test falls back to): one all-reduce per all-loci step through the
    library's callback (RCCL on the driver's box, the framework's gloo collective here), the per-locus sweeps by the persistent
    kernel ("hybrid"); p2p = True, the DEFAULT at N > 1: the sums exchanged inside the persistent kernel through peer-mapped
    mailboxes, the program's moves"""
    d, err = run_bench(["--scaling", scaling] + (["--p2p-sums"] if p2p else ["--no-p2p"]))
    assert d["n_gpus"] == 2 and d["steps"] == 6 and d["scaling"] == scaling and d["value"] > 0
    assert d["allreduce_check"] == "ok"
    assert ("p2p" in d["allreduce"]["tape"]) == p2p, (d["allreduce"], err[-1500:])
    smp, tp = d["device_resident_sampler"], d["likelihood_only"]
    if p2p:
        assert "persistent kernel" in d["allreduce"]["sampler"] and smp["implementation"].startswith("persistent"), d["allreduce"]
        assert smp["moves"].startswith("the program's")
    else:
        assert "mailboxes" not in d["allreduce"]["sampler"] and smp["kind"] == "hybrid", d["allreduce"]
    assert d["roofline"]["frac"] > 0 and "iter_kernel" in d["roofline"]["kernel"] and d["cpu_baseline"] is None
    # strong: the 1 500 loci are shared out (750 each); weak: 1 500 per rank
    total = 1500 if scaling == "strong" else 3000
    assert smp["loci_total"] == total and tp["loci_total"] == total
    assert smp["n_gpus"] == 2 and smp["iterations_per_s"] > 0 and 0.2 < smp["acceptance"] < 0.9
    assert d["value"] == (smp["iterations_per_s"] if scaling == "strong" else smp["iterations_per_s_10k_loci"])
    assert d["value_" + scaling] == d["value"]
    assert tp["roofline"]["frac"] > 0 and tp["roofline"]["proposal_steps"] >= tp["roofline"]["launches"]


def test_two_rank_bench_line_config3_runs_the_program_s_moves():
    """--config c3 on two ranks: the generic sampler's loci dealt out (strong scaling), BPP's own iteration on every rank — the
    ranks' decision kernels take THETA / TAU / MIX from sums that went through the collective"""
    d, err = run_bench(["--config", "c3", "--loci", "400", "--no-tape", "--projection-iters", "2", "--no-scale-projection"])
    smp = d["device_resident_sampler"]
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["value"] > 0, err[-1500:]
    assert smp["moves"].startswith("the program's") and smp["moves_short"] == "program" and smp["kind"] == "generic", smp["moves"]
    assert smp["loci_total"] == 400 and 0.1 < smp["acceptance"] < 0.9
    assert smp["theta_gibbs_draws_generic"]["proposed"] > 0


def test_eight_rank_bench_line():
    """BASELINE's eight-GPU world size, run with four ranks: `bench.py --gpus 4` as the driver launches it (torch.distributed.run,
    one rank per GPU — here four ranks on device 0 over gloo: a shared GPU machine lets at most six processes open a GPU at once,
    the pytest process among them) with the exchange over
    the collective (--no-p2p: persistent kernels of several processes on ONE GPU are not reliably co-resident, so the in-kernel
    exchange at this world size is left to real hardware): n_gpus 4, the whole-job rate under both scalings (weak = four data sets,
    strong = one dealt out by the reference's zig-zag over four parts), the tape's all-reduce self-check over four ranks."""
    d, err = run_bench(["--loci", "320", "--no-scale-projection", "--no-p2p"], world=4)
    assert d["n_gpus"] == 4 and d["scaling"] == "weak" and d["value"] == d["value_weak"] > 0, err[-1500:]
    assert d["value_strong"] and d["value_strong"] > 0, (d.get("scaling_other_mode"), err[-1500:])
    assert d["allreduce_check"] == "ok"
    smp, tp = d["device_resident_sampler"], d["likelihood_only"]
    assert smp["n_gpus"] == 4 and smp["loci_total"] == 4*320 and tp["loci_total"] == 4*320
    assert d["scaling_other_mode"]["scaling"] == "strong" and d["scaling_other_mode"]["loci_total"] == 320
    assert smp["kind"] == "hybrid"


def test_two_rank_bench_line_carries_both_scalings():
    """without --scaling: `value` = the config's own mode (c2: weak) and the other mode's sampler rate is measured in the same run"""
    d, err = run_bench(["--no-tape"])
    assert d["scaling"] == "weak" and d["value"] == d["value_weak"] > 0
    assert "persistent kernel" in d["allreduce"]["sampler"], d["allreduce"]          # (no flag: the in-kernel exchange)
    assert d["value_strong"] and d["value_strong"] > 0, (d.get("scaling_other_mode"), err[-1500:])
    assert d["scaling_other_mode"]["scaling"] == "strong" and d["scaling_other_mode"]["loci_total"] == 1500


def test_one_gpu_bench_line_quick():
    """the full run (`python bench.py --gpus 1 --steps K --warmup W --full`) with the side sections switched off but the
    likelihood-only tape: the last stdout line is the compact object with the contract's keys, `roofline` with its three
    fractions and a warning-free `frac`, the full record goes where --full-record says"""
    import tempfile
    full_path = os.path.join(tempfile.mkdtemp(prefix="bench1_"), "full.json")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", "--loci", "2000", "--full", "--no-cpu-baseline",
           "--no-other-configs", "--no-host-control", "--no-scale-projection", "--no-uniform-kernel", "--full-record", full_path]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1]
    assert len(last) <= 8192
    d = json.loads(last)
    full = json.load(open(full_path))
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 2 and d["value"] == full["value"] > 0
    assert d["dtype"] == "f64" and d["data"] == "synthetic" and d["higher_is_better"] is True and d["config"]["workload"]
    rl = d["roofline"]
    assert rl["bound"] == "hbm" and 0 < rl["frac"] < 0.79 and "warning" not in rl and rl["frac_codes"] <= rl["frac"] and rl["flops_frac"] > 0
    smp = full["device_resident_sampler"]
    assert smp["kind"] == "persistent" and smp["moves"].startswith("the program's") and smp["step_lengths_after_burnin"]["gage"] > 0
    lo = d["likelihood_only"]
    assert lo["it_s"] > 0 and lo["frac_codes"] <= lo["frac"]


def test_one_gpu_plain_bench_line_is_the_headline_alone():
    """the driver's own form (`python bench.py --gpus 1 --steps K --warmup W`): the device-resident sampler alone (no tape, no CPU
    baseline, no other configuration), and the state its timed iterations leave (--dump-outputs) is the one the --full run's
    headline leaves after the likelihood-only tape ran on the same loci"""
    import tempfile
    import numpy as np
    tmp = tempfile.mkdtemp(prefix="bench_plain_")
    common = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", "--loci", "2000"]
    r = subprocess.run(common + ["--full-record", os.path.join(tmp, "plain.json"), "--dump-outputs", os.path.join(tmp, "plain")],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    full = json.load(open(os.path.join(tmp, "plain.json")))
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert line["metric"] == full["metric"] == base["metric"] and line["unit"] == "iterations/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f64" and line["steps"] == 4 and line["warmup"] == 2
    smp = full["device_resident_sampler"]
    assert line["value"] == full["value"] == smp["iterations_per_s_10k_loci"] > 0 and line["ms_per_step"] == smp["ms_per_step"] > 0
    assert smp["kind"] == "persistent" and smp["steps"] == 4 and "device_uniform_kernel" not in smp
    for k in ("likelihood_only", "cpu_baseline", "cpu_tape_replay", "reference_program_on_host", "statistical_efficiency",
              "other_configs", "host_control_in_c", "scale_projection"):
        assert full[k] is None, k
    assert "section: likelihood-only tape" not in r.stderr
    # the same headline after the full run's tape section: the same inputs, the same iterations, the same state
    r2 = subprocess.run(common + ["--full", "--no-cpu-baseline", "--no-other-configs", "--no-host-control", "--no-scale-projection",
                                  "--no-uniform-kernel", "--full-record", os.path.join(tmp, "full.json"), "--dump-outputs", os.path.join(tmp, "full")],
                        cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0, r2.stderr[-2000:]
    assert json.load(open(os.path.join(tmp, "full.json")))["likelihood_only"]["steps"] == 4
    names = sorted(f for f in os.listdir(os.path.join(tmp, "plain")) if f.endswith(".npy"))
    assert "locus_lnl.npy" in names and names == sorted(f for f in os.listdir(os.path.join(tmp, "full")) if f.endswith(".npy"))
    for f in names:
        assert np.array_equal(np.load(os.path.join(tmp, "plain", f)), np.load(os.path.join(tmp, "full", f)), equal_nan=True), f
