"""Posterior of the UNMODIFIED reference program (oracle/_ref/bpp, A00, HKY + discrete-gamma rates with 4 categories) on a
synthetic 12-locus 4-species data set — the known answer for the closed-form models' parameter moves (one exchangeability
against its reference entry under the program's Dirichlet prior {2,4,2,2,4,2}, locus.c:3168-3354; the frequencies,
locus.c:2782; alpha, prop_gamma.c:52-224) next to the tree moves (tests/test_closedform_host.py, tests/test_gpu_closedform.py).

    python tests/golden/make_golden_hky.py         ->  tests/golden/hky_posterior.json   (about a minute)

The data come from bpp_amd.synth (model "hky", kappa 3, seed 79; the tests regenerate them), are written as a sequential
PHYLIP file + Imap + control file, and bpp runs 4 000 burn-in + 40 000 x 2 iterations with thetaprior = gamma 2 500,
tauprior = gamma 2 600, alphaprior = 1 1 4, model = hky, print = 1 0 0 0 1 (the last flag: every locus's kappa and
frequencies into <job>.locus_<i>_params_sample.txt), from program seeds 1 and 2.  Only summaries go into the fixture: per
quantity — every theta, every tau, lnL, every locus's log kappa — mean and sd of the two runs pooled, and each run's own.
The script asserts that the two runs agree within HALF the test's bars (mean within 0.15 sd, sd within 0.125 sd); if they do
not, lengthen the run.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from bpp_amd import synth          # noqa: E402

CFG = dict(nloci=12, sites=300, taxa=4, seed=79, theta=0.004, kappa=3.0, theta_prior=(2.0, 500.0), tau_prior=(2.0, 600.0),
           alpha_prior=(1.0, 1.0), rate_cats=4, burnin=4000, sampfreq=2, nsample=40000, program_seeds=(1, 2))
HALF_MEAN, HALF_SD = 0.15, 0.125


def run(data, seed):
    names = "ABCD"
    with tempfile.TemporaryDirectory() as td:
        with open(os.path.join(td, "seqs.txt"), "w") as f:
            for d in data:
                seqs = ["".join(ch * int(w) for ch, w in zip(s, d["weights"])) for s in d["seqs"]]
                f.write(f"4 {len(seqs[0])}\n")
                for nm, s in zip(names, seqs):
                    f.write(f"s^{nm.lower()}  {s}\n")
                f.write("\n")
        with open(os.path.join(td, "imap.txt"), "w") as f:
            f.write("".join(f"{c.lower()} {c}\n" for c in names))
        with open(os.path.join(td, "a00.ctl"), "w") as f:
            f.write(f"seed = {seed}\nseqfile = seqs.txt\nImapfile = imap.txt\njobname = out\nspeciesdelimitation = 0\n"
                    "speciestree = 0\nspecies&tree = 4  A B C D\n                  1 1 1 1\n"
                    "                 (((A, B), C), D);\nusedata = 1\n"
                    f"nloci = {CFG['nloci']}\nmodel = hky\nalphaprior = {CFG['alpha_prior'][0]:g} {CFG['alpha_prior'][1]:g} {CFG['rate_cats']}\n"
                    "cleandata = 0\n"
                    f"thetaprior = gamma {CFG['theta_prior'][0]:g} {CFG['theta_prior'][1]:g}\n"
                    f"tauprior = gamma {CFG['tau_prior'][0]:g} {CFG['tau_prior'][1]:g}\nfinetune = 1\nprint = 1 0 0 0 1\n"
                    f"burnin = {CFG['burnin']}\nsampfreq = {CFG['sampfreq']}\nnsample = {CFG['nsample']}\n")
        subprocess.run([os.path.join(ROOT, "oracle", "_ref", "bpp"), "--cfile", "a00.ctl"], cwd=td, check=True,
                       stdout=subprocess.DEVNULL)
        rows = [ln.rstrip("\n").split("\t") for ln in open(os.path.join(td, "out.mcmc.txt"))]
        head = [h.strip() for h in rows[0]]
        body = np.array([[float(x) for x in r] for r in rows[1:]])
        cols = {h: body[:, c] for c, h in enumerate(head) if c > 0}
        for i in range(CFG["nloci"]):
            lr = [ln.rstrip("\n").split("\t") for ln in open(os.path.join(td, f"out.locus_{i + 1}_params_sample.txt"))]
            lh = [h.strip() for h in lr[0]]
            k = lh.index("kappa")
            cols[f"logkappa:{i}"] = np.log(np.array([float(r[k]) for r in lr[1:] if len(r) > k]))
    return cols


def main():
    data = synth.make_dataset(CFG["nloci"], CFG["sites"], CFG["taxa"], "hky", CFG["rate_cats"], seed=CFG["seed"], theta=CFG["theta"], kappa=CFG["kappa"])
    runs = [run(data, s) for s in CFG["program_seeds"]]
    post, worst = {}, (0.0, 0.0)
    for h in runs[0]:
        a, b = runs[0][h], runs[1][h]
        both = np.concatenate([a, b])
        sd = float(both.std())
        dm, ds = abs(a.mean() - b.mean())/sd, abs(a.std() - b.std())/sd
        worst = (max(worst[0], dm), max(worst[1], ds))
        assert dm < HALF_MEAN and ds < HALF_SD, (h, a.mean(), b.mean(), a.std(), b.std(), "the two program seeds disagree: lengthen the run")
        post[h] = dict(mean=float(both.mean()), sd=sd, runs=[dict(mean=float(x.mean()), sd=float(x.std())) for x in (a, b)])
    out = dict(config=CFG, columns=list(runs[0]), samples=[len(next(iter(r.values()))) for r in runs],
               seeds_apart=dict(mean_in_sd=worst[0], sd_in_sd=worst[1]), posterior=post)
    with open(os.path.join(HERE, "hky_posterior.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: (round(v["mean"], 5), round(v["sd"], 5)) for k, v in post.items()}, indent=1))
    print("seeds apart (in sd): mean %.3f, sd %.3f" % worst)


if __name__ == "__main__":
    main()
