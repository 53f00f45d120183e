#!/usr/bin/env python
"""Dev tool (GPU box): what the multi-task lasso's fused x-update buys, per right-hand sides per pass (MT_RHS).

    bench_mtlasso.py [--n 100000] [--p 10000] [--m 2,4,8] [--rhs 2,4,8,12] [--nlambda 10] [--steps 3] [--warmup 1] [--stride 5]

Device-resident inputs; for every m one model per MT_RHS value is prepared (LassoPlan), and the prepared plans are run in turn, round
after round (warmup + steps rounds), so that a drift of the clocks falls on every setting alike.  Reported per (m, NR), median and
[min, max] over the steps:
  xupdate_us    event-timed duration of ALL x-update passes of one iteration (start of the first pass to the end of the last,
                every stride-th iteration sampled: PROFILE_STRIDE, admm_stats.xupdate_ms_avg);
  iteration_us  loop time / iterations as the library reports them (admm_stats.t_loop, total_iter);
  rest_us       iteration_us - xupdate_us: tall_mt_tail_kernel plus the launch gaps (beside tall_tail_kernel's 5.4 us + gaps).
NR = 2 is m launches of the two-vector arithmetic and schedule: the baseline.  `lasso` is the single-response Lasso on response 0 --
symv2_lower_kernel itself, one launch per iteration -- so m x its xupdate_us is what m independent fits stream.
Every NR must give byte-identical coefficients; the script checks that.  Prints one JSON line.

The tail kernel's own time is not in these figures (rest_us holds the launch gaps too, and the events cost something themselves).  It
comes from a kernel trace of a run of its own, one m per process since the kernel has one name, without event sampling:
    rocprofv3 --kernel-trace --stats -f csv -d DIR -- python scripts/bench_mtlasso.py --n 12000 --m 8 --rhs 0 --stride 0
(--rhs 0: the automatic value only; n does not enter the tail) and the row of tall_mt_tail_kernel in DIR's kernel statistics."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before libadmm_hip: one HIP runtime per process)
import numpy as np  # noqa: E402
from admm_amd import DevicePtr, _lib, admm_lasso, admm_mtlasso  # noqa: E402
from admm_amd.api import LassoPlan  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=100000)
ap.add_argument("--p", type=int, default=10000)
ap.add_argument("--m", default="2,4,8")
ap.add_argument("--rhs", default=",".join(str(v) for v in _lib.MT_RHS_BUILT))
ap.add_argument("--nlambda", type=int, default=10)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--stride", type=int, default=5)
a = ap.parse_args()
n, p = a.n, a.p
ms = [int(v) for v in a.m.split(",")]
rhs = [int(v) for v in a.rhs.split(",")]
mmax = max(ms)

dev = torch.device("cuda", 0)
g = torch.Generator(device=dev)
g.manual_seed(5)
xt = torch.empty((p, n), dtype=torch.float64, device=dev)          # p x n row-major == n x p column-major
chunk = max(1, (1 << 27) // n)
for c0 in range(0, p, chunk):
    c1 = min(p, c0 + chunk)
    xt[c0:c1] = torch.randn((c1 - c0, n), generator=g, device=dev, dtype=torch.float64) * 2
nact = min(1000, p // 10)
B = torch.zeros((mmax, p), dtype=torch.float64, device=dev)
B[:, :nact] = torch.rand((mmax, nact), generator=g, device=dev, dtype=torch.float64)
Yt = B @ xt + torch.randn((mmax, n), generator=g, device=dev, dtype=torch.float64)      # m x n row-major == n x m column-major
torch.cuda.synchronize()
xp, yp = DevicePtr(xt.data_ptr()), DevicePtr(Yt.data_ptr())


def med(v):
    v = sorted(v)
    return [round(v[len(v) // 2], 2), [round(v[0], 2), round(v[-1], 2)]]


def measure(models):
    """{name: model} -> {name: (figures, coefficients)}: every model prepared once, then all of them run in turn, round after round."""
    plans = {}
    with _lib.options(PROFILE_STRIDE=a.stride):
        for name, (model, opts) in models.items():
            with _lib.options(**opts):
                plans[name] = LassoPlan(model)
    xs, its = {k: [] for k in plans}, {k: [] for k in plans}
    last = {}
    for r in range(a.warmup + a.steps):
        for name, plan in plans.items():
            fit = plan.run()
            st = fit.stats
            if r >= a.warmup:
                xs[name].append(st["xupdate_ms_avg"] * 1e3)
                its[name].append(st["t_loop"] / st["total_iter"] * 1e6)
            last[name] = (st, fit.beta_dense)
    out = {}
    for name, plan in plans.items():
        plan.close()
        st, beta = last[name]
        x, it = med(xs[name]), med(its[name])
        out[name] = ({"xupdate_us": x, "iteration_us": it, "rest_us": round(it[0] - x[0], 2), "iterations": int(st["total_iter"]),
                      "samples": int(st["xupdate_samples"])}, beta)
    return out


out = {"n": n, "p": p, "nlambda": a.nlambda, "steps": a.steps, "stride": a.stride}
out["lasso"] = measure({"lasso": (admm_lasso(xp, yp, n=n, p=p).penalty(nlambda=a.nlambda), {})})["lasso"][0]
for m in ms:
    got = measure({f"NR={nr}": (admm_mtlasso(xp, yp, n=n, p=p, m=m).penalty(nlambda=a.nlambda), {"MT_RHS": nr}) for nr in rhs})
    row, first = {}, None
    for nr in rhs:
        row[f"NR={nr}"], beta = got[f"NR={nr}"]
        if nr > 0:
            row[f"NR={nr}"]["passes"] = -(-2 * m // nr)
        if first is None:
            first = beta
        elif first.tobytes() != beta.tobytes():
            raise SystemExit(f"m = {m}: MT_RHS = {nr} changed the coefficients")
    out[f"m={m}"] = row
print(json.dumps(out))
