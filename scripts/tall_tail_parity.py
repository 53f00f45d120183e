#!/usr/bin/env python
"""Dev tool (GPU box): sha256 digests of everything the tall path's three tail kernels write, case by case, so that two builds of the
library can be held to each other bit for bit.

    timeout -k 10 300 python scripts/tall_tail_parity.py [--ranks 2] > digests.jsonl

Run it from a tree of each build (the script uses the package of the tree it lies in) on the same machine and compare the two outputs:
every line must be equal.  One JSON line per case: the digests of the lambda grid, beta, niter, the decision trace (which holds the norm
sums of every iteration) and the iterate dump (x, z, y, adj_z, adj_y of every iteration).

Seeded data, n = 600, p = 230 (8 workgroups of 32 coordinates, the last ragged), 20 lambdas; every case with the gemv and with the sym
x-update unless it says otherwise -- the two instantiations of each tail.  --ranks 2: also the row-sharded Lasso over the three exchange
forms (generic all-reduce, PEER, PEER1), two processes on one device through tests/dist_worker.py, each under a time limit of its own;
those lines hold what the worker stores (grid, beta, niter, trace)."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

N, P, NLAM = 600, 230, 20
CAP = 1 << 14          # trace / dump records: more than any case below takes


def sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(str((a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()[:16]


def data(m=1):
    rng = np.random.default_rng(2024)
    x = rng.standard_normal((N, P)) * 2.0
    B = np.zeros((P, m))
    B[:25] = rng.uniform(size=(25, m))
    Y = x @ B + rng.standard_normal((N, m))
    return np.asfortranarray(x), (Y[:, 0].copy() if m == 1 else np.asfortranarray(Y))


def labels(sizes):
    assert sum(sizes) == P
    return np.repeat(np.arange(len(sizes)), sizes)


FOURS = [4] * 57 + [2]                         # groups of 4 (and the remainder)
BIG = [3] * 20 + [70] + [3] * 33 + [1]         # one group of 70 among groups of 3: three passes of one workgroup, the last ragged


def weights(sizes):
    return np.random.default_rng(3).choice([0.0, 0.5, 1.0], size=len(sizes), p=[0.15, 0.35, 0.5])


def run_case(name, model, **opts):
    from admm_amd import _lib
    from admm_amd.api import LassoPlan
    with _lib.options(**opts):
        plan = LassoPlan(model)
        plan.enable_trace(CAP)
        plan.enable_state(CAP)
        fit = plan.run()
        trace, state = plan.read_trace(), plan.read_state()
        plan.close()
    assert len(trace) < CAP, name
    print(json.dumps({"case": name, "opts": opts, "records": int(len(trace)), "niter_max": int(np.max(fit.niter)), "lambda": sha(fit.lambda_),
                      "beta": sha(fit.beta_dense), "niter": sha(fit.niter), "trace": sha(trace), "state": sha(state)}), flush=True)


def single_device():
    from admm_amd import admm_boxenet, admm_enet, admm_grplasso, admm_lasso, admm_mtlasso, admm_sgl
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from box_oracle import box_pattern
    x, y = data()
    lower, upper, factors = box_pattern(P)
    u = np.random.default_rng(31).uniform(0.5, 2.0, P)
    pen = dict(nlambda=NLAM)
    for xu in ("gemv", "sym"):
        run_case("lasso", admm_lasso(x, y).penalty(**pen), XUPDATE=xu)
        run_case("enet alpha=0.5", admm_enet(x, y).penalty(alpha=0.5, **pen), XUPDATE=xu)
        run_case("lasso maxit=30", admm_lasso(x, y).penalty(**pen).opts(maxit=30), XUPDATE=xu)        # several lambdas end on the cap
        for gname, sizes in (("fours", FOURS), ("big70", BIG)):
            g = labels(sizes)
            run_case(f"grplasso {gname}", admm_grplasso(x, y, g).penalty(group_weights=weights(sizes), **pen), XUPDATE=xu)
            run_case(f"sgl alpha=0.5 {gname}", admm_sgl(x, y, g, alpha=0.5).penalty(l1_weights=u, **pen), XUPDATE=xu)
        run_case("sgl alpha=1", admm_sgl(x, y, labels(FOURS), alpha=1.0).penalty(l1_weights=u, **pen), XUPDATE=xu)
        run_case("boxenet lasso prox", admm_boxenet(x, y, lower, upper).penalty(penalty_factor=factors, **pen), XUPDATE=xu)
        run_case("boxenet alpha=0.5", admm_boxenet(x, y, lower, upper).penalty(alpha=0.5, penalty_factor=factors, **pen), XUPDATE=xu)
    run_case("lasso refined", admm_lasso(x, y).penalty(**pen), XUPDATE="sym", REFINE="1")
    for m in (1, 3, 4, 5, 16):                 # one chunk partly filled, one full, the second with one live slot, all chunks full
        xm, Y = data(m)
        run_case(f"mtlasso m={m}", admm_mtlasso(xm, Y).penalty(**pen))


def sharded(nranks):
    """Row-sharded Lasso, one line per exchange form, through the worker of tests/test_gpu_dist2.py."""
    worker = os.path.join(ROOT, "tests", "dist_worker.py")
    forms = (("allreduce", "shm", {}), ("PEER1", "peer", {}), ("PEER", "peer", {"ADMM_HIP_TEST_RESIDENT_WGS": "4"}))
    for name, backend, extra in forms:
        with tempfile.TemporaryDirectory(prefix="tailparity") as wd:
            env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **extra)
            procs = [subprocess.Popen([sys.executable, worker, backend, str(r), str(nranks), wd, "tallshard300"], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(nranks)]
            outs = []
            try:
                for pr in procs:
                    outs.append(pr.communicate(timeout=120)[0])
            finally:
                for pr in procs:
                    if pr.poll() is None:
                        pr.kill()
            for r, pr in enumerate(procs):
                if pr.returncode != 0:      # nothing more is started on the device after a failure
                    raise SystemExit(f"sharded {name}: rank {r} ended with {pr.returncode}\n{outs[r][-2000:]}")
            res = [dict(np.load(os.path.join(wd, f"result.{r}.npz"))) for r in range(nranks)]
        for r in res[1:]:
            assert all(sha(r[k]) == sha(res[0][k]) for k in ("beta", "niter", "trace")), name
        print(json.dumps({"case": f"sharded lasso {name}", "ranks": nranks, "exchange_variant": int(res[0]["exchange_variant"]),
                          "records": int(len(res[0]["trace"])), "lambda": sha(res[0]["lam"]), "beta": sha(res[0]["beta"]),
                          "niter": sha(res[0]["niter"]), "trace": sha(res[0]["trace"])}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", type=int, default=0)
    a = ap.parse_args()
    if a.ranks > 1:            # first: the workers open the device themselves, this process has not yet
        sharded(a.ranks)
    single_device()
