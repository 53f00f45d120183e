#!/usr/bin/env python
"""Dev tool (GPU box): the C4 consensus Lasso (n = 10^4, p = 10^5, K = 8 row blocks, 3 lambdas down to 0.3 lambda_max) through plain
admm_hip_parlasso, the default single-device path against the in-process multi-device mode (option PAR_DEVICES).  With more than one
device the mode runs PAR_DEVICES=all; on a one-GPU box it runs PAR_DEVICES=0,0 -- two ranks as threads on the SAME device, which
measures what the mode itself costs (threads, per-rank contexts, the two-launch PEER exchange, two copies of the setup on one GPU),
not any scaling.  Prints one JSON line per leg and a summary.
Usage: bench_parallel_devices.py [repeats] [out.json]"""
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import numpy as np  # noqa: E402
from admm_amd import DevicePtr, admm_lasso, last_parallel_layout, load, options  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
out_path = sys.argv[2] if len(sys.argv) > 2 else None
n, p, K = 10000, 100000, 8
lib = load()
ndev = lib.admm_hip_device_count()
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev); g.manual_seed(4)
xt = torch.empty((p, n), dtype=torch.float64, device=dev)           # p x n row-major == n x p column-major
chunk = max(1, (1 << 27) // n)
for c0 in range(0, p, chunk):
    c1 = min(p, c0 + chunk)
    xt[c0:c1] = torch.randn((c1 - c0, n), generator=g, device=dev, dtype=torch.float64) * 2
b = torch.zeros(p, dtype=torch.float64, device=dev)
b[:100] = torch.rand(100, generator=g, device=dev, dtype=torch.float64)
y = b @ xt + torch.randn(n, generator=g, device=dev, dtype=torch.float64)
torch.cuda.synchronize()


def leg(devices):
    model = admm_lasso(DevicePtr(xt.data_ptr()), DevicePtr(y.data_ptr()), n=n, p=p).penalty(nlambda=3, lambda_min_ratio=0.3).parallel(K).opts(maxit=4000)
    rows = []
    with options(PAR_DEVICES=devices):
        model.fit()                                                  # warm-up (code objects, pools, the rank threads' streams)
        for _ in range(reps):
            t0 = time.time()
            fit = model.fit()
            lib.admm_hip_device_synchronize()
            wall = time.time() - t0
            it = int(np.sum(fit.niter))
            st = fit.stats
            rows.append(dict(wall_s=wall, t_loop=st["t_loop"], setup_s=st["t_total"] - st["t_loop"], iters=it,
                             iters_per_s=it / st["t_loop"] if st["t_loop"] > 0 else None))
        layout = last_parallel_layout()
    best = min(rows, key=lambda r: r["wall_s"])
    res = dict(par_devices=devices or "unset", layout=layout, niter=[int(v) for v in fit.niter], beta_nnz=int(np.count_nonzero(fit.beta_dense)),
               exchange_variant=int(fit.stats["exchange_variant"]), best=best, runs=rows)
    print(json.dumps(res), flush=True)
    return res, fit


base, fb = leg(None)
mode = "all" if ndev > 1 else "0,0"
par, fp = leg(mode)
summary = dict(workload=f"C4 consensus Lasso n={n} p={p} K={K}, device input, plain admm_hip_parlasso", devices_visible=ndev,
               compare=f"default vs PAR_DEVICES={mode}",
               meaning=("scaling over the visible devices" if ndev > 1 else
                        "ONE GPU: both ranks share device 0 -- the overhead of the in-process mode (threads, contexts, two-launch PEER form, "
                        "two setups on one device), not a multi-GPU speed-up"),
               default_wall_s=base["best"]["wall_s"], par_wall_s=par["best"]["wall_s"],
               default_iters_per_s=base["best"]["iters_per_s"], par_iters_per_s=par["best"]["iters_per_s"],
               default_setup_s=base["best"]["setup_s"], par_setup_s=par["best"]["setup_s"],
               same_niter=base["niter"] == par["niter"],
               max_abs_beta_diff=float(np.abs(fb.beta_dense.astype(np.float64) - fp.beta_dense.astype(np.float64)).max()))
print(json.dumps(summary), flush=True)
if out_path:
    with open(out_path, "w") as f:
        json.dump(dict(summary=summary, default=base, par=par), f, indent=1)
