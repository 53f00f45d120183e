#!/usr/bin/env python
"""Measure admm_hip_logit_enet_cv / admm_hip_poisson_cv (K-fold cross-validation of the penalised GLMs on ONE setup) against what a user
does without them: F + 1 separate admm_hip_logit_enet / admm_hip_poisson calls, the full data and F training sets whose rows are
gathered on the HOST, each call paying its own upload, standardisation, Gram matrix, inverse and transpose.

Shape: n = 50000, k = 8, fp64, HOST-resident input on both sides, intercept TRUE, F = 5 (row i in fold i mod 5), five lambda =
f lambda_1 at alpha = 1, f = 0.5, 0.3, 0.2, 0.1, 0.05 (lambda_1 the largest over the k columns of the FULL data, the same five values in
every call), p = 1000 ... 4000, the default stop rule (eps 1e-4, maxit 10000): 240 fits per cross-validation call, 40 per separate call.
Data: scripts/bench_logit_enet.py's design; logistic labels as there, Poisson counts from the same linear scores.

Per p and loss, on the serial route (QUANT_SLOTS=1) and the automatic one: one warm-up and `--repeats` timed repeats of
  * "cv": the wall time of the one cross-validation call;
  * "separate": the summed wall time of the F + 1 public calls on rows gathered beforehand -- the host gather (NumPy fancy indexing into
    column-major copies) is timed once and reported beside it, since the user pays it too.
Median and spread (max - min) / median of each, their ratio, and the iteration totals of both sides (a fold's fit in the one call is
not the separate call's fit: that one re-standardises its rows and has c^2 = its own row count).
Prints one JSON line per measurement.
Usage: bench_glm_cv.py [--n N --p P[,P...] --k K --folds F --repeats R --loss logit[,poisson]]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=50000)
ap.add_argument("--p", default="1000,2000,3000,4000")
ap.add_argument("--k", type=int, default=8)
ap.add_argument("--folds", type=int, default=5)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--loss", default="logit,poisson")
args = ap.parse_args()
n, k, F = args.n, args.k, args.folds
PS = [int(v) for v in str(args.p).split(",")]
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before libadmm_hip)
import admm_amd as A  # noqa: E402
from admm_amd import options  # noqa: E402

dev = torch.device("cuda", 0)
FRACTIONS = (0.5, 0.3, 0.2, 0.1, 0.05)
BUILD = {"logit": (A.admm_logit_enet, A.admm_logit_enet_cv), "poisson": (A.admm_poisson, A.admm_poisson_cv)}


def make(p):
    """-> host arrays: x (n x p, column-major), logistic labels and Poisson counts (n x k, column-major)"""
    g = torch.Generator(device=dev)
    g.manual_seed(123)
    xt = torch.empty((p, n), dtype=torch.float64, device=dev)
    chunk = max(1, (1 << 27) // n)
    for c0 in range(0, p, chunk):
        c1 = min(p, c0 + chunk)
        xt[c0:c1] = torch.randn((c1 - c0, n), generator=g, device=dev, dtype=torch.float64) * 2.0
    lab = torch.empty((k, n), dtype=torch.float64, device=dev)
    cnt = torch.empty((k, n), dtype=torch.float64, device=dev)
    for c in range(k):
        bc = (2 * torch.rand(p, generator=g, device=dev, dtype=torch.float64) - 1) / p ** 0.5
        score = 0.5 * (bc @ xt)
        lab[c] = (torch.rand(n, generator=g, device=dev, dtype=torch.float64) < torch.sigmoid(score - 0.8 + 1.6 * c / max(1, k - 1))).to(torch.float64)
        cnt[c] = torch.poisson(torch.exp(0.5 * score - 0.5 + 1.5 * c / max(1, k - 1)), generator=g)
    torch.cuda.synchronize()
    out = np.asfortranarray(xt.cpu().numpy().T), np.asfortranarray(lab.cpu().numpy().T), np.asfortranarray(cnt.cpu().numpy().T)
    del xt, lab, cnt
    torch.cuda.empty_cache()
    return out


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


fid = np.arange(n) % F
for p in PS:
    x, lab, cnt = make(p)
    t0 = time.perf_counter()
    train_x = [np.asfortranarray(x[fid != f]) for f in range(F)]
    t_gather_x = time.perf_counter() - t0
    for loss in args.loss.split(","):
        public, cv = BUILD[loss]
        Y = lab if loss == "logit" else cnt
        t0 = time.perf_counter()
        train_y = [np.asfortranarray(Y[fid != f]) for f in range(F)]
        t_gather = t_gather_x + time.perf_counter() - t0
        lam = [f * float(public(x, Y, 1.0).lambda_one().max()) for f in FRACTIONS]
        print(json.dumps({"loss": loss, "p": p, "lambda": lam, "host_gather_s": t_gather}), flush=True)
        for slots in (1, None):
            walls = {"cv": [], "separate": []}
            iters, variant = {}, {}
            for r in range(args.repeats + 1):
                with options(QUANT_SLOTS=slots):
                    t0 = time.perf_counter()
                    fit = cv(x, Y, lam, alpha=1.0, nfolds=F).fit()
                    t_cv = time.perf_counter() - t0
                    t0 = time.perf_counter()
                    parts = [public(x, Y, lam, alpha=1.0).fit()] + [public(train_x[f], train_y[f], lam, alpha=1.0).fit() for f in range(F)]
                    t_sep = time.perf_counter() - t0
                if r:
                    walls["cv"].append(t_cv)
                    walls["separate"].append(t_sep)
                iters = {"cv": int(fit.niter.sum() + fit.fold_niter.sum()), "separate": int(sum(int(q.niter.sum()) for q in parts))}
                variant = {"cv": int(fit.stats["xupdate_variant"]), "separate": int(parts[0].stats["xupdate_variant"])}
                assert np.array_equal(fit.beta, parts[0].beta) and np.array_equal(fit.niter, parts[0].niter)      # the f = 0 slot is the public call
            med = {name: statistics.median(v) for name, v in walls.items()}
            print(json.dumps({"loss": loss, "p": p, "n": n, "k": k, "folds": F, "route": "serial" if slots == 1 else "auto", "variant": variant, "repeats": args.repeats,
                              "cv_wall_s": med["cv"], "cv_spread": spread(walls["cv"]), "separate_wall_s": med["separate"], "separate_spread": spread(walls["separate"]),
                              "cv_over_separate": med["cv"] / med["separate"], "cv_over_separate_with_gather": med["cv"] / (med["separate"] + t_gather),
                              "host_gather_s": t_gather, "fit_iterations": iters, "idx_min": fit.idx_min.tolist(), "idx_1se": fit.idx_1se.tolist(),
                              "t_loop_cv": fit.stats["t_loop"], "walls": walls}), flush=True)
        del train_y
    del x, lab, cnt, train_x
