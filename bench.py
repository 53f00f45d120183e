#!/usr/bin/env python
"""Headline benchmark: ADMM iterations/s of the tall Lasso lambda path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]

A plain run sets up, runs W warm-up steps, times K steps and prints one JSON line (`ms_per_step` = milliseconds per timed
step).  `--full` adds everything else described below: the steady-state setup (`setup_s`, `sec_to_eps`), `cpu_baseline`, the
other BASELINE configs (`configs`) and the side measurements.  `--dump-outputs DIR` writes what the last timed step returned
(lambda.npy, beta.npy, niter.npy; see dump_outputs) so that two builds can be compared output for output.

Workload (BASELINE.json configs[1], SURVEY.md section 8d "C2"): admm_lasso tall, n=100000,
p=10000, fp32 solver arithmetic, automatic 100-lambda grid (lambda_min_ratio 1e-4), warm-started,
standardize = intercept = TRUE, eps_abs = eps_rel = 1e-5, synthetic Gaussian data generated in
HBM (X ~ N(0, 2^2), beta* = U(0,1) on the first 1000 coordinates, y = X beta* + N(0,1)).

A "step" is one pass of the hot path: the complete warm-started lambda path (the loop of
Lasso.cpp:97-124 -> FADMMBase::solve) from a cold start on the resident data.  The one-time
preparation the reference does before that loop (convert, DataStd, X'y, Gram, Spectra, Cholesky)
runs once before the timed region and is reported separately as `setup_s_cold` (with --full a
second time, steady state, as `setup_s`); `sec_to_eps[_cold]` = that setup + one path.
value = sum of ADMM iterations of the K timed steps (over all ranks) divided
by the max-over-ranks wall time of the timed region.

N > 1 (one process per GPU; `python bench.py --gpus N` started WITHOUT a launcher re-executes itself under
`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1`, and a WORLD_SIZE that
disagrees with --gpus is refused -- a line saying n_gpus: 1 can not come out of a --gpus 8 call):
  * primary line = the headline workload itself with its x-update spread over the N GPUs (1/N of the
    inverse's lower-triangle tiles per rank, ONE all-reduce of 2p floats per ADMM iteration, RCCL or the
    hand-written peer-mapped exchange -- the better of the two valid runs) -> "scaling": "strong".  A sharded run
    only counts when its communicator really held N ranks, the ranks agreed on every iteration count and every
    lambda converged; otherwise the line falls back to the replica figure and says so (`parallelism`).
  * `replicas_weak`: N independent replicas of the single-GPU solver (what the reference's serial solver offers,
    SURVEY.md 8e "replicas only"), no data-path collective.
  * with --full, side objects, each from time-limited child processes with their own rendezvous so that a failing exchange can
    never take the primary line down: `exchange_self_check` (both back-ends against a closed-form sum, first),
    `consensus` (BASELINE configs[3]: 8 row blocks spread over the ranks, one grouped all-reduce of p floats per
    iteration), `wide_column_sharded` (configs[2] with its columns spread over the ranks, all-reduce of n floats).

Extra objects on the JSON line: `roofline` for the dominant kernel (the x-update mat-vec: 2*p^2
algorithmic bytes per launch for the symmetric lower-triangle kernel, 4*p^2 for the full-matrix
one; durations from kernel-exact HIP start/stop events recorded by the library on its own stream
inside the timed region) and, with --full, `cpu_baseline` (the compiled C restatement of the same loop,
oracle/c, timed on the host cores on a bounded sample: the reference's one-core configuration,
and a best-effort all-core cached-inverse variant beside it).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12   # B/s, MI355X spec (MI355X_MICROARCH.md)
# test hook: take every multi-rank branch (process groups, all-reduces, consensus children) with WORLD_SIZE=1
FORCE_DIST = os.environ.get("ADMM_BENCH_FORCE_DIST") == "1"
# test hook: ranks share devices (local_rank modulo the device count) and the control plane runs over gloo -- the self-spawned
# N > 1 launch executed on a one-GPU box (tests/test_gpu_bench_children.py)
OVERSUBSCRIBE = os.environ.get("ADMM_BENCH_OVERSUBSCRIBE") == "1"


def self_spawn(a):
    """`python bench.py --gpus N` (N > 1) without a launcher: become `torch.distributed.run` with N ranks on this node (what the
    driver's own command line does), after checking that N devices exist.  Never returns."""
    import socket
    import subprocess
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"], capture_output=True, text=True)
    try:
        ndev = int(r.stdout.strip().splitlines()[-1])
    except Exception:                                        # noqa: BLE001
        raise SystemExit("bench.py: could not count the visible GPUs: " + (r.stderr or r.stdout)[-300:])
    if ndev < a.gpus and not OVERSUBSCRIBE:
        raise SystemExit(f"bench.py: --gpus {a.gpus} but only {ndev} device(s) visible: refusing to run (no n_gpus: {ndev} line for a --gpus {a.gpus} call)")
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    # the launcher's own option parser looks at the script's arguments too (and rejects e.g. `--n` as an ambiguous abbreviation of its
    # own options): only the three flags of the driver's contract travel on the command line, the full argument list in the environment
    os.environ["ADMM_BENCH_ARGV"] = json.dumps(sys.argv[1:])
    argv = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}", "--master-addr", "127.0.0.1",
            "--master-port", str(port), os.path.abspath(__file__), "--gpus", str(a.gpus), "--steps", str(a.steps), "--warmup", str(a.warmup)]
    sys.stderr.write("[bench] --gpus %d without a launcher: re-executing as %s\n" % (a.gpus, " ".join(argv[1:9])))
    sys.stderr.flush()
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.execv(sys.executable, argv)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--p", type=int, default=10000)
    ap.add_argument("--m", type=int, default=1000, help="non-zeros in beta*")
    ap.add_argument("--nlambda", type=int, default=100)
    ap.add_argument("--seed", type=int, default=123)
    ap.add_argument("--full", action="store_true",
                    help="also run everything beside the headline figure: the steady-state setup, cpu_baseline, the other BASELINE configs "
                         "and the side measurements (without it: setup, warm-up, the timed steps and the result line only)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write what the last timed step returned (lambda, beta, niter) to DIR/<name>.npy")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="budget of the cpu_baseline loop (0 disables)")
    ap.add_argument("--profile-stride", type=int, default=32, help="time every k-th x-update launch with HIP events")
    ap.add_argument("--consensus-seconds", type=float, default=180.0,
                    help="time limit of the side measurement of the consensus solver (0 disables it)")
    ap.add_argument("--shard-seconds", type=float, default=200.0,
                    help="time limit of each sharded child run at N > 1 (0 disables them: replicas only)")
    ap.add_argument("--config-seconds", type=float, default=150.0,
                    help="time limit of each child run of the other BASELINE configs at N = 1 (C3 wide, C4 consensus, C5 LAD / BP, parbp; 0 disables them)")
    ap.add_argument("--cpu-config-seconds", type=float, default=6.0,
                    help="budget of EACH timed CPU leg (1 thread, all threads) of the other configs (0 disables their cpu_baseline)")
    ap.add_argument("--exchanges", default="rccl,peer", help="exchange back-ends of the sharded / consensus child runs at N > 1 (comma-separated: rccl, peer)")
    ap.add_argument("--side-shapes", default="", help=argparse.SUPPRESS)      # test hook: "n,p" of the consensus child and "n,p,nl" of the wide child, ";"-separated (tests/test_gpu_bench_children.py)
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    if os.environ.get("ADMM_BENCH_ARGV") and "--child" not in sys.argv:      # a self-spawned rank (self_spawn): the original argument list
        a = ap.parse_args(json.loads(os.environ["ADMM_BENCH_ARGV"]))
    else:
        a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    return a


DUMP_BUDGET_BYTES = 64 * 10**6


def dump_outputs(fit, out_dir):
    """--dump-outputs: what LassoPlan.run() handed its caller in the last timed step -- the lambda grid, the (p+1) x nlambda
    coefficients (intercept first) and the iteration counts -- as DIR/lambda.npy (float64), DIR/beta.npy (float32) and DIR/niter.npy
    (float64).  Above 64 MB in all, beta.npy holds a fixed seeded sample of its rows and DIR/beta_rows.npy (float64) says which."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"lambda": np.asarray(fit.lambda_, dtype=np.float64), "niter": np.asarray(fit.niter, dtype=np.float64)}
    beta = np.ascontiguousarray(fit.beta_dense, dtype=np.float32)
    room = DUMP_BUDGET_BYTES - 4096 - sum(v.nbytes for v in arrays.values())      # 4096: the .npy headers
    if beta.nbytes > room:
        row_bytes = beta.shape[1] * beta.itemsize + 8                # a kept row: its floats plus its index in beta_rows.npy
        rows = np.sort(np.random.default_rng(0).choice(beta.shape[0], room // row_bytes, replace=False))
        beta = np.ascontiguousarray(beta[rows])
        arrays["beta_rows"] = rows.astype(np.float64)
    arrays["beta"] = beta
    for name, v in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), v)


def cpu_baseline(p, nlambda, budget_s, seed, n_full=None):
    """The reference's loop on the host cores, compiled C (oracle/c/admm_tall_cpu.c through oracle/ctall.py), on a
    bounded sample of the same workload: same p, n_s = 2p rows of the same synthetic distribution (the per-iteration
    cost depends on p only), the first lambdas of the same automatic grid.  Two configurations:
      value        faithful: Cholesky factor + two triangular solves per iteration on ONE core -- Eigen's LLT::solve is
                   serial and Lasso.cpp:1 defines EIGEN_DONT_PARALLELIZE, so this is what the reference runs;
      best_effort  cached-inverse mat-vec over all host threads (OpenMP) -- what a tuned CPU build of this repository's
                   own x-update would do; not the reference's arithmetic.
    Setup (Gram, Lanczos, Cholesky, inverse) uses NumPy/LAPACK and is not part of either rate."""
    import numpy as np
    import scipy.linalg as sla
    # the all-core leg: threads pinned and spread over the cores, pages first-touched by the thread that streams them (oracle/c)
    os.environ.setdefault("OMP_PROC_BIND", "spread")
    os.environ.setdefault("OMP_PLACES", "cores")
    from oracle import ctall
    from oracle.datastd import DataStd
    from oracle.entry import _lambda_grid
    from oracle.solvers import LassoTall
    rng = np.random.default_rng(seed)
    n_s = 2 * p
    m = max(1, p // 10)
    X = (rng.standard_normal((n_s, p), dtype=np.float32) * np.float32(2.0))
    b = np.zeros(p, dtype=np.float32)
    b[:m] = rng.uniform(size=m).astype(np.float32)
    Y = (X @ b + rng.standard_normal(n_s, dtype=np.float32)).astype(np.float32)
    X = np.asfortranarray(X)
    std = DataStd(n_s, p, True, True, np.float32)
    std.standardize(X, Y)
    t0 = time.time()
    solver = LassoTall(X, Y, 1e-5, 1e-5)
    lam = _lambda_grid(solver.lambda0, n_s, std.scaleY, nlambda, 1e-4)
    lam_int = np.array([np.float64(np.float32(l * n_s / np.float64(std.scaleY))) for l in lam])
    solver.init(lam_int[0], -1.0)
    L = np.asfortranarray(np.tril(solver.chol[0]))
    t_setup = time.time() - t0
    del X

    def timed(factor, mode, nthreads, budget):
        # calibrate on the first two lambdas, then run as many lambdas (from a cold start) as fit the budget
        _, it, secs = ctall.tall_loop(factor, solver.XY, lam_int[:2], solver.rho, 1e-5, 1e-5, 10000, None, mode, nthreads)
        per_iter = secs / max(1, int(it.sum()))
        k = 2
        est = int(it.sum())
        while k < nlambda and (est + 25) * per_iter < budget:      # ~25 iterations per further lambda on this grid
            k += 1
            est += 25
        _, it, secs = ctall.tall_loop(factor, solver.XY, lam_int[:k], solver.rho, 1e-5, 1e-5, 10000, None, mode, nthreads)
        return int(it.sum()) / secs, int(it.sum()), secs, k

    v1, it1, s1, k1 = timed(L, 0, 1, 0.6 * budget_s)
    threads = ctall.max_threads()
    t0 = time.time()
    Li = sla.solve_triangular(L.astype(np.float64), np.eye(p), lower=True, check_finite=False)
    Minv = np.asfortranarray((Li.T @ Li).astype(np.float32))
    del Li
    t_inv = time.time() - t0
    vb, itb, sb, kb = timed(Minv, 1, threads, 0.4 * budget_s)
    # sec_to_eps needs a CPU counterpart of the one-time setup too: measured here on the n_s-row sample (NumPy float Gram +
    # Lanczos + LAPACK Cholesky, all host threads), and -- labelled as such -- extrapolated to the full n (the Gram is linear
    # in n, everything else depends on p only).  The reference itself forms the Gram with single-threaded Eigen.
    setup_full_est = None
    if n_full:
        t_gram_s = max(t_setup - 2.0, 0.5 * t_setup)            # Cholesky + Lanczos at p = 10^4 take ~2 s of it
        setup_full_est = t_gram_s * (float(n_full) / n_s) + (t_setup - t_gram_s)
    return {"value": v1, "unit": "iterations/s", "cores": 1, "kind": "port", "setup_s": t_setup, "setup_sample_rows": n_s,
            "setup_s_full_n_extrapolated": setup_full_est,
            "sample": f"C restatement of FADMMBase::solve + ADMMLassoTall (oracle/c/admm_tall_cpu.c, gcc -O3), float Cholesky factor + 2 "
                      f"triangular solves per iteration on ONE thread (the reference's configuration: serial LLT::solve, "
                      f"EIGEN_DONT_PARALLELIZE), p={p}, n_sample={n_s} rows (per-iteration cost depends on p only), first {k1} of "
                      f"{nlambda} lambdas of the automatic grid from a cold start: {it1} iterations in {s1:.1f} s; NumPy/LAPACK setup "
                      f"(Gram + Lanczos + Cholesky) {t_setup:.1f} s not included",
            "best_effort": {"value": vb, "unit": "iterations/s", "cores": int(threads),
                            "sample": f"same loop with the x-update as a cached-inverse symmetric mat-vec spread over {threads} OpenMP "
                                      f"threads (OMP_PROC_BIND=spread, OMP_PLACES=cores, matrix pages first-touched by the thread that "
                                      f"streams them; not the reference's arithmetic), first {kb} lambdas: {itb} iterations in {sb:.2f} s; "
                                      f"forming the inverse took {t_inv:.1f} s (not included)"}}


def _child_setup(backend):
    """Common prologue of the side-measurement children: own gloo process group (control plane), the library's
    communicator over `backend` in {"rccl", "peer"} (data plane)."""
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    multi = world > 1 or FORCE_DIST
    import torch
    import torch.distributed as dist
    if OVERSUBSCRIBE:
        local_rank = local_rank % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if multi:
        dist.init_process_group(backend="gloo")
    from admm_amd import load
    from admm_amd import dist as adist
    lib = load()
    assert lib.admm_hip_set_device(local_rank) == 0
    if multi:
        adist.init_comm_backend_from_torch(backend, dev)
    elif backend == "peer":
        adist.init_comm_peer(1, 0, lambda mine: mine)
    else:
        adist.init_comm(1, 0)
    return rank, world, multi, torch, dist, dev, adist


def _child_teardown(plan, adist, dist, multi):
    plan.close()
    if multi:
        dist.barrier()                                   # nobody unmaps / destroys while a peer may still push
    adist.finalize_comm()
    if multi:
        dist.destroy_process_group()


def _ranks_agree(niter, torch, dist, multi, dev):
    """Replicated decisions: every rank must report the same iteration counts (a broken exchange shows up here first)."""
    if not multi:
        return True
    t = torch.tensor([int(v) for v in niter], dtype=torch.int64, device=dev)
    hi, lo = t.clone(), t.clone()
    dist.all_reduce(hi, op=dist.ReduceOp.MAX)
    dist.all_reduce(lo, op=dist.ReduceOp.MIN)
    return bool(torch.equal(hi, lo))


def _max_over_ranks(v, torch, dist, multi):
    if not multi:
        return v
    t = torch.tensor([v], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t[0])


def exchcheck_child(a, backend, out_path):
    """First thing at N > 1: the exchange layer on its own, before any solver depends on it.  Every rank contributes a known vector
    (floats and doubles, rank-dependent), the in-place sum all-reduce of `backend` runs three times (the slot parity of the PEER /
    SHM protocols alternates), and every rank compares with the closed-form sum.  The first 8-GPU run of this tree is also the first
    execution of every nccl* call of comm.hip with more than one rank in the communicator and the first PEER exchange across xGMI:
    this child says WHICH of the two works there, the measurements that follow keep going either way (run_side_measurement)."""
    rank, world, multi, torch, dist, dev, adist = _child_setup(backend)
    import numpy as np
    nf, nd = 100003, 5
    ok, worst = True, 0.0
    for rep in range(3):
        f = ((np.arange(nf) % 977) * 1e-3 + rank + 0.25 * rep).astype(np.float32)
        d = (np.arange(nd) * 1e-3 + 2.0 * rank + rep).astype(np.float64)
        ef = sum(((np.arange(nf) % 977) * 1e-3 + r + 0.25 * rep).astype(np.float32).astype(np.float64) for r in range(world))
        ed = sum((np.arange(nd) * 1e-3 + 2.0 * r + rep) for r in range(world))
        adist.allreduce_host(f, d)
        ferr = float(np.abs(f.astype(np.float64) - ef).max() / np.abs(ef).max())
        derr = float(np.abs(d - ed).max() / np.abs(ed).max())
        worst = max(worst, ferr, derr)
        ok = ok and ferr < 1e-6 * world and derr < 1e-14 * world
    allok = True
    if multi:
        t = torch.tensor([1 if ok else 0], dtype=torch.int64)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        allok = bool(int(t[0]) == 1)
    if rank == 0:
        with open(out_path, "w") as f_:
            json.dump({"exchange": backend, "ranks": world, "all_ranks_correct": allok, "worst_relative_error_rank0": worst,
                       "payload": "%d floats + %d doubles, 3 exchanges" % (nf, nd)}, f_)
    if multi:
        dist.barrier()
    adist.finalize_comm()
    if multi:
        dist.destroy_process_group()


def consensus_child(a, backend, out_path):
    """Side measurement (own processes, own process group): BASELINE configs[3]-shaped consensus Lasso
    `admm_lasso(x, y)$parallel(K)`, n=10000, p=100000, K = number of ranks, one row block per GPU, rows
    sharded over ranks, one exchange (p floats + 3 doubles) per ADMM iteration over `backend`."""
    rank, world, multi, torch, dist, dev, adist = _child_setup(backend)
    from admm_amd import DevicePtr
    n, p = 10000, 100000
    if a.side_shapes:
        n, p = (int(v) for v in a.side_shapes.split(";")[0].split(","))
    K = 8 if 8 % world == 0 else world                   # BASELINE configs[3]: 8 row blocks, spread over the ranks (8 / N per GPU): total work fixed as N grows
    lo, hi = adist.row_partition(n, K, world, rank)
    nl = hi - lo
    gb = torch.Generator(device="cpu"); gb.manual_seed(a.seed)
    beta_true = torch.zeros(p, dtype=torch.float64)
    beta_true[:100] = torch.rand(100, generator=gb, dtype=torch.float64)
    beta_true = beta_true.to(dev)
    g = torch.Generator(device=dev); g.manual_seed(a.seed + 1000 + rank)
    xt = torch.randn((p, nl), generator=g, device=dev, dtype=torch.float64) * 2.0      # p x nl row-major == nl x p column-major
    y = beta_true @ xt + torch.randn(nl, generator=g, device=dev, dtype=torch.float64)
    torch.cuda.synchronize()
    t0 = time.time()
    # a lambda range on which the consensus iteration CONVERGES (rho = lambda_1 / K is slow: the README problem takes 339
    # iterations): the rate must not be that of runs cut off at maxit
    plan = adist.DistLassoPlan(DevicePtr(xt.data_ptr()), DevicePtr(y.data_ptr()), n, p, K, nlambda=3, lambda_min_ratio=0.3,
                               n_local=nl, maxit=4000)
    setup_s = time.time() - t0
    del xt
    plan.run()                                           # warm-up (RCCL lazy initialisation)
    if multi:
        dist.barrier()
    fit = plan.run()
    iters = int(fit.stats["total_iter"])
    loop_s = _max_over_ranks(fit.stats["t_loop"], torch, dist, multi)
    agree = _ranks_agree(fit.niter, torch, dist, multi, dev)
    if rank == 0:
        rows = n // K
        bytes_per_gpu = (K // world) * (4.0 * rows * p + 4.0 * rows * rows)      # per block: A streamed ONCE (A_k's_k; A_k rhs_k by recurrence + gather, round 5) + the cached (AA'+rho I)^-1
        res = {"workload": "admm_lasso$parallel(8) n=10000 p=100000 (BASELINE configs[3]), 8 row blocks spread over the GPUs, 3 lambdas down to 0.3 lambda_max, run to convergence (maxit 4000)",
               "scaling": "strong",
               "converged": bool(all(int(v) <= 4000 for v in fit.niter)), "ranks_agree_on_niter": agree,
               "exchange": backend, "n_gpus": world, "ranks_in_communicator": adist.comm_info()[0], "K": K, "iterations": iters, "loop_s": loop_s,
               "iters_per_s": iters / loop_s, "ms_per_iter": loop_s / iters * 1e3, "setup_s": setup_s,
               "alg_bytes_per_gpu_per_iter": bytes_per_gpu, "achieved_GBps_per_gpu": bytes_per_gpu * iters / loop_s / 1e9,
               "allreduce_payload_bytes": 4 * p + 24, "niter": [int(v) for v in fit.niter]}
        with open(out_path, "w") as f:
            json.dump(res, f)
    _child_teardown(plan, adist, dist, multi)


def tallshard_child(a, backend, out_path):
    """The headline workload itself (BASELINE configs[1]: tall Lasso n x p, 100-lambda path) with its x-update spread
    over the ranks (admm_hip_lasso_plan_create_dist, nthread = 0): rows of the synthetic problem sharded for the setup
    (split-K Gram + all-reduce), 1/N of the inverse's lower-triangle tiles per rank and ONE all-reduce of 2p floats per
    ADMM iteration over `backend`.  Total work is fixed as N grows: strong scaling."""
    rank, world, multi, torch, dist, dev, adist = _child_setup(backend)
    from admm_amd import DevicePtr
    n, p = a.n, a.p
    lo, hi = n * rank // world, n * (rank + 1) // world
    nl = hi - lo
    gb = torch.Generator(device="cpu"); gb.manual_seed(a.seed)
    beta_true = torch.zeros(p, dtype=torch.float64)
    beta_true[:a.m] = torch.rand(a.m, generator=gb, dtype=torch.float64)
    beta_true = beta_true.to(dev)
    g = torch.Generator(device=dev); g.manual_seed(a.seed + 2000 + rank)
    xt = torch.empty((p, nl), dtype=torch.float64, device=dev)
    chunk = max(1, (1 << 27) // max(nl, 1))
    for c0 in range(0, p, chunk):
        c1 = min(p, c0 + chunk)
        xt[c0:c1] = torch.randn((c1 - c0, nl), generator=g, device=dev, dtype=torch.float64) * 2.0
    y = beta_true @ xt + torch.randn(nl, generator=g, device=dev, dtype=torch.float64)
    torch.cuda.synchronize()
    from admm_amd import options as _options
    _options.set(PROFILE_STRIDE=a.profile_stride)           # (the child's _child_setup has loaded the library: the environment is not read any more)
    t0 = time.time()
    plan = adist.DistLassoPlan(DevicePtr(xt.data_ptr()), DevicePtr(y.data_ptr()), n, p, 0, nlambda=a.nlambda, lambda_min_ratio=1e-4,
                               n_local=nl)
    setup_s = time.time() - t0
    del xt
    torch.cuda.empty_cache()
    for _ in range(max(1, a.warmup)):
        plan.run()
    if multi:
        dist.barrier()
    t0 = time.time()
    iters, loop_ms, xms, xsamp = 0, 0.0, 0.0, 0
    for _ in range(a.steps):
        fit = plan.run()
        iters += int(fit.stats["total_iter"])
        loop_ms += fit.stats["loop_ms_events"]
        xms += fit.stats["xupdate_ms_avg"] * fit.stats["xupdate_samples"]
        xsamp += int(fit.stats["xupdate_samples"])
    elapsed = _max_over_ranks(time.time() - t0, torch, dist, multi)
    setup_s = _max_over_ranks(setup_s, torch, dist, multi)
    agree = _ranks_agree(fit.niter, torch, dist, multi, dev)
    if rank == 0:
        x_ms = xms / max(1, xsamp)
        res = {"workload": "admm_lasso tall path (BASELINE configs[1]), x-update sharded over the ranks", "exchange": backend,
               "ranks_agree_on_niter": agree, "all_lambdas_converged": bool(int(max(fit.niter)) <= 10000),
               "n_gpus": world, "ranks_in_communicator": adist.comm_info()[0], "scaling": "strong", "steps": a.steps,
               "iterations_per_step": iters / a.steps, "elapsed_s": elapsed, "iters_per_s": iters / elapsed,
               "us_per_iter": elapsed / iters * 1e6, "loop_ms_events_per_step": loop_ms / a.steps, "setup_s": setup_s,
               "xupdate_share_avg_launch_ms": x_ms, "xupdate_share_alg_bytes": 2.0 * p * p / world,
               "xupdate_share_GBps": (2.0 * p * p / world) / (x_ms * 1e-3) / 1e9 if x_ms > 0 else None,
               "allreduce_payload_bytes": 8 * ((p + 127) // 128 * 128), "niter_first": [int(v) for v in fit.niter[:8]]}
        with open(out_path, "w") as f:
            json.dump(res, f)
    _child_teardown(plan, adist, dist, multi)


def widecols_child(a, backend, out_path):
    """BASELINE configs[2] (admm_lasso wide n=2000, p=200000, ADMMLassoWide) with its COLUMNS spread over the ranks
    (admm_hip_lasso_dist_cols): local X_i't / prox / active set, one all-reduce of A x (n floats) per iteration over
    `backend`.  Total work fixed as N grows: strong scaling.  A 20-lambda path (the full 100 at N = 1 takes 0.45 s)."""
    rank, world, multi, torch, dist, dev, adist = _child_setup(backend)
    from admm_amd import DevicePtr
    n, p, nl_wide = 2000, 200000, 20
    if a.side_shapes:
        n, p, nl_wide = (int(v) for v in a.side_shapes.split(";")[1].split(","))
    lo, hi = adist.col_partition(p, world, rank)
    pl = hi - lo
    gb = torch.Generator(device="cpu"); gb.manual_seed(a.seed)
    beta_true = torch.zeros(p, dtype=torch.float64)
    beta_true[:100] = torch.rand(100, generator=gb, dtype=torch.float64)
    noise = torch.randn(n, generator=gb, dtype=torch.float64)
    # every rank needs the full y = X beta* + noise: the first 100 columns (all non-zeros of beta*) are generated identically everywhere
    gh = torch.Generator(device=dev); gh.manual_seed(a.seed + 3000)
    xhead = torch.randn((100, n), generator=gh, device=dev, dtype=torch.float64) * 2.0
    y = beta_true[:100].to(dev) @ xhead + noise.to(dev)
    g = torch.Generator(device=dev); g.manual_seed(a.seed + 3001 + rank)
    xt = torch.randn((pl, n), generator=g, device=dev, dtype=torch.float64) * 2.0      # pl x n row-major == n x pl column-major
    if lo < 100:
        xt[:100 - lo] = xhead[lo:100]
    torch.cuda.synchronize()
    from admm_amd._lib import AdmmOpts, AdmmStats, check, load
    import ctypes
    import numpy as np
    lib = load()
    nl = nl_wide
    lam_out = np.zeros(nl); beta = np.zeros((p + 1, nl), dtype=np.float32, order="F"); niter = np.zeros(nl, dtype=np.int32)
    o = AdmmOpts(10000, 1e-5, 1e-5, -1.0)

    def run():
        stats = AdmmStats()
        check(lib.admm_hip_lasso_dist_cols(ctypes.c_void_p(xt.data_ptr()), ctypes.c_void_p(y.data_ptr()), n, pl, p, lo, 1, None, 0, nl, 0.01,
                                           1, 1, -1.0, ctypes.byref(o), lam_out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                           beta.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), niter.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                           ctypes.byref(stats)))
        return stats.as_dict()

    run()                                                # warm-up
    if multi:
        dist.barrier()
    st = run()
    iters = int(st["total_iter"])
    loop_s = _max_over_ranks(st["t_loop"], torch, dist, multi)
    agree = _ranks_agree(niter, torch, dist, multi, dev)
    if rank == 0:
        res = {"workload": "admm_lasso wide n=%d p=%d (BASELINE configs[2]), columns sharded over the ranks, %d-lambda path" % (n, p, nl),
               "exchange": backend, "ranks_agree_on_niter": agree, "all_lambdas_converged": bool(int(niter.max()) <= 10000), "n_gpus": world, "ranks_in_communicator": adist.comm_info()[0], "scaling": "strong", "iterations": iters,
               "loop_s": loop_s, "iters_per_s": iters / loop_s, "us_per_iter": loop_s / iters * 1e6,
               "setup_s": st["t_total"] - st["t_loop"], "allreduce_payload_bytes": 4 * n, "niter_first": [int(v) for v in niter[:8]],
               "persist_iter": int(st.get("persist_iter", 0)), "exchange_variant": int(st.get("exchange_variant", 0))}
        with open(out_path, "w") as f:
            json.dump(res, f)
    if multi:
        dist.barrier()
    adist.finalize_comm()
    if multi:
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------------------------
# The other BASELINE.json configs on ONE GPU (N = 1), each in its own time-limited child process, each with its roofline
# and -- timed in the parent on the host cores -- its cpu_baseline (the NumPy restatement of the same loop, oracle/solvers.py,
# on the same shape for a bounded number of iterations, with 1 BLAS thread = the reference's configuration and with all of them).
CONFIGS = {
    "c3": dict(workload="admm_lasso wide n=2000 p=200000, 100-lambda path (BASELINE configs[2])", dtype="f32"),
    "c4": dict(workload="admm_lasso$parallel(8) n=10000 p=100000, 8 row blocks on ONE GPU (BASELINE configs[3] at N = 1), 3 lambdas down to 0.3 lambda_max, run to convergence", dtype="f32"),
    "c5lad": dict(workload="admm_lad n=50000 p=5000 (BASELINE configs[4])", dtype="f64"),
    "c5bp": dict(workload="admm_bp n=5000 p=50000 (BASELINE configs[4], transposed as the reference's API requires: p > n)", dtype="f64"),
    "c5parbp": dict(workload="admm_bp$parallel(8) n=5000 p=50000, column-block sharing ADMM, 8 blocks on ONE GPU", dtype="f64"),
}


def _gen_device(torch, dev, g, n, p, sd, m, dense_beta=False, noise=True):
    xt = torch.empty((p, n), dtype=torch.float64, device=dev)
    chunk = max(1, (1 << 27) // n)
    for c0 in range(0, p, chunk):
        c1 = min(p, c0 + chunk)
        xt[c0:c1] = torch.randn((c1 - c0, n), generator=g, device=dev, dtype=torch.float64) * sd
    b = torch.zeros(p, dtype=torch.float64, device=dev)
    if dense_beta:
        b[:] = torch.rand(p, generator=g, device=dev, dtype=torch.float64)
    else:
        idx = torch.randperm(p, generator=g, device=dev)[:m] if not noise else torch.arange(m, device=dev)
        b[idx] = torch.rand(m, generator=g, device=dev, dtype=torch.float64)
    y = b @ xt
    if noise:
        y = y + torch.randn(n, generator=g, device=dev, dtype=torch.float64)
    torch.cuda.synchronize()
    return xt, y, b


def config_child(a, name, out_path):
    """One of the other BASELINE configs on cuda:0, inputs resident in HBM, a warm-up fit and a timed one.  The rate is
    iterations / seconds of the ADMM loop (admm_stats.t_loop: host clock around a device sync; loop_ms_events: HIP events on the
    solver's stream around the same loop), setup reported beside it; `roofline` from SURVEY.md section 8(d)'s per-iteration
    algorithmic bytes."""
    import torch
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    import numpy as np
    from admm_amd import DevicePtr, admm_bp, admm_lad, admm_lasso, load
    lib = load()
    assert lib.admm_hip_set_device(0) == 0
    g = torch.Generator(device=dev)
    g.manual_seed(a.seed)
    extra = {}
    survey_bytes = None
    if name == "c3":
        n, p = 2000, 200000
        xt, y, _ = _gen_device(torch, dev, g, n, p, 2.0, 100)
        model = admm_lasso(DevicePtr(xt.data_ptr()), DevicePtr(y.data_ptr()), n=n, p=p).penalty(nlambda=100)
        model.fit()
        fit = model.fit()
        niter = fit.niter.astype(np.int64)
        reg = sum(int(sum(1 for c in range(k) if (c + 1) & c == 0 and ((c + 1) & 0x55555555))) for k in niter)
        tot = int(niter.sum())
        # a regular iteration streams X once (4 n p); EVERY iteration reads the columns of the current support twice
        # (X_S' t in the x-update, X_S x_S for A x: 2 * 4 n nS).  The kernels do not record nS per iteration; it is taken per lambda
        # as the mean of the support sizes the lambda starts from (the previous lambda's final support: warm start) and ends with
        # -- known exactly from the returned coefficients -- times that lambda's iteration count.
        nnz = np.count_nonzero(fit.beta_dense[1:, :], axis=0).astype(np.float64)
        nnz_start = np.concatenate([[0.0], nnz[:-1]])
        supp_bytes = float((8.0 * n * 0.5 * (nnz_start + nnz) * niter).sum())
        screened = int(fit.stats["xupdate_variant"])            # 0 no, 1 fp16 copy, 2 8-bit code
        reg_bytes = {0: 4.0, 1: 2.0, 2: 1.0}[screened] * n * p      # what a regular step of THIS solver streams (safe screening)
        bytes_iter = (reg_bytes * reg + supp_bytes) / max(1, tot)
        survey_bytes = (4.0 * n * p * reg + supp_bytes) / max(1, tot)
        extra = {"regular_iterations": reg, "nnz_last_lambda": int(nnz[-1]), "persist_iter": int(fit.stats["persist_iter"]),
                 "support_bytes_share": supp_bytes / (reg_bytes * reg + supp_bytes),
                 "regular_steps_screened": {0: False, 1: "fp16 copy", 2: "8-bit code"}[screened],
                 "kernel": "wide_x_kernel / wide_rows_persist_kernel (x-update of ADMMLassoWide)",
                 "bytes_note": "per ITERATION averaged over the path: the regular steps' stream + 8 n nS on every step (nS per lambda = mean of its "
                               "starting and final support sizes).  Screened regular steps (DESIGN.md section 3) prove 'stays zero' from a 1- or 2-byte "
                               "copy of X and stream np / 2np bytes, not the 4np SURVEY section 8(d) prices: `achieved` counts what this solver's iteration "
                               "has to move, `survey_8d_*` the reference's arithmetic on the same iterations.  The path is latency-bound: 96 % of its "
                               "iterations are active-set steps of ~1 MB inside the persistent stretch"}
    elif name == "c4":
        n, p, K = 10000, 100000, 8
        xt, y, _ = _gen_device(torch, dev, g, n, p, 2.0, 100)
        model = admm_lasso(DevicePtr(xt.data_ptr()), DevicePtr(y.data_ptr()), n=n, p=p).penalty(nlambda=3, lambda_min_ratio=0.3).parallel(K).opts(maxit=4000)
        model.fit()
        fit = model.fit()
        # round 5, one-pass Woodbury workers: ONE stream of every A_k per iteration (A_k's_k) + the cached inverses; A_k rhs_k comes
        # from rows_k-sized recurrences and a gather over the non-zero columns of z (4 n nnz(z) bytes, not recorded per iteration
        # and not counted: lower bound).  SURVEY section 8(d) prices the reference's two streams: quoted beside it.
        bytes_iter = 4.0 * n * p + 4.0 * K * (n / K) ** 2
        survey_bytes = 8.0 * n * p + 4.0 * K * (n / K) ** 2
        extra = {"K": K, "niter": [int(v) for v in fit.niter], "converged": bool(all(int(v) <= 4000 for v in fit.niter)),
                 "kernel": "gemv_t_batch_kernel (A_k' s_k of the 8 Woodbury workers, PADMMLasso.h:22-30; A_k rhs_k by recurrence + gather_batch_kernel)",
                 "bytes_note": "per ITERATION, HIP events around the loop: one stream of A (4np) + the inverses; the gather over supp(z) is not counted (lower bound)"}
    elif name == "c5lad":
        n, p = 50000, 5000
        xt, y, _ = _gen_device(torch, dev, g, n, p, 2.0, p, dense_beta=True)
        model = admm_lad(DevicePtr(xt.data_ptr()), DevicePtr(y.data_ptr()), intercept=False, n=n, p=p)
        model.fit()
        fit = model.fit()
        # round 6, one-pass form: the rows of X stream ONCE per iteration (x = X s, prox, dual, X'z_new, X'y_new from the same rows;
        # X'vec from p-vectors); SURVEY section 8(d) prices the reference's two products with X
        onepass = int(fit.stats["xupdate_variant"]) == 1
        bytes_iter = (8.0 if onepass else 16.0) * n * p + 8.0 * p * p
        survey_bytes = 16.0 * n * p + 8.0 * p * p
        extra = {"kernel": "lad_rows_kernel (x = X s, z, y, norms, X'z, X'y in one pass over the rows of X) + gemv_t_kernel<double> ((X'X)^-1 u)" if onepass
                           else "gemv_t_kernel<double> (X' v, (X'X)^-1 t, X s: ADMMLAD.h:75-76)",
                 "one_pass": onepass,
                 "bytes_note": "per ITERATION (all launches of one ADMM iteration), HIP events around the loop: X once (8np) + the inverse (8p^2) in the one-pass form"
                               if onepass else "per ITERATION (all launches of one ADMM iteration), HIP events around the loop"}
    elif name in ("c5bp", "c5parbp"):
        n, p = 5000, 50000
        xt, y, b = _gen_device(torch, dev, g, n, p, 1.0, 500, noise=False)
        model = admm_bp(DevicePtr(xt.data_ptr()), DevicePtr(y.data_ptr()), n=n, p=p)
        if name == "c5parbp":
            model = model.parallel(8)
        model.fit()
        fit = model.fit()
        beta = np.asarray(fit.beta.todense()).ravel()
        err = beta - b.cpu().numpy()
        extra = {"recovery_error_range": [float(err.min()), float(err.max())]}
        if name == "c5bp":
            # round 5, one-pass form: only B'w streams (8np); B vec from n-sized recurrences + a gather over the non-zeros of z
            # (8 n nnz(z) bytes, not counted: lower bound).  SURVEY section 8(d) prices the reference's two products (16np).
            bytes_iter = 8.0 * n * p
            survey_bytes = 16.0 * n * p
            extra["kernel"] = "gemv_t_kernel<double> (B' w, B = L^-1 A: ADMMBP.h:60-67; B vec by recurrence + bp_gather_kernel)"
            extra["bytes_note"] = "per ITERATION, HIP events around the loop: one stream of B (8np); the gather over supp(z) is not counted (lower bound)"
        else:
            it = int(fit.stats["total_iter"])
            reg = (it + 9) // 10
            screened = int(fit.stats["xupdate_variant"]) >= 4     # regular iterations screened through the fp16 copy of A (2np instead of 8np)
            bytes_iter = (2.0 if screened else 8.0) * n * p * reg / max(it, 1)
            survey_bytes = 8.0 * n * p * reg / max(it, 1)
            extra.update({"regular_iterations": reg, "nnz": int(np.count_nonzero(beta)), "regular_steps_screened": "fp16 copy" if screened else False,
                          "kernel": "sbp_xreg_screen_kernel / sbp_gs_kernel" if screened else "sbp_xreg_kernel / sbp_xact_kernel",
                          "bytes_note": "regular-step stream only (every 10th iteration; lower bound): the fp16 copy of A when screened (DESIGN.md section 3), "
                                        "A itself (8np, `survey_8d_*`) otherwise"})
    else:
        raise SystemExit("unknown config " + name)
    st = fit.stats
    it = int(st["total_iter"])
    loop_s = float(st["t_loop"])
    ev_s = float(st["loop_ms_events"]) * 1e-3
    t_iter = (ev_s if ev_s > 0 else loop_s) / max(it, 1)
    achieved = bytes_iter / t_iter
    res = dict(CONFIGS[name])
    res.update({"value": it / loop_s, "unit": "iterations/s", "iterations": it, "loop_s": loop_s, "loop_s_events": ev_s, "n_gpus": 1,
                "setup_s": float(st["t_total"]) - loop_s, "sec_to_eps": float(st["t_total"]),
                "roofline": {"bound": "hbm", "kernel": extra.pop("kernel", None), "achieved": achieved / 1e9, "peak": HBM_PEAK / 1e9, "unit": "GB/s",
                             "frac": achieved / HBM_PEAK, "traffic": None, "algorithmic_bytes_per_iteration": bytes_iter,
                             "avg_iteration_ms": t_iter * 1e3, "note": extra.pop("bytes_note", "per ITERATION (all launches of one ADMM iteration), HIP events around the loop")}})
    try:          # PMC counters cannot be collected inside this run: quote the committed per-iteration measurement of this config
        # (scripts/capture_pmc_configs.sh) while the source files of its loop kernels are unchanged -- else null: re-profile
        import hashlib
        ent = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json"))).get("configs", {}).get(name)
        if ent:
            h = hashlib.sha256()
            for f in ent["source_files"]:
                h.update(open(os.path.join(ROOT, "admm_amd", "csrc", f), "rb").read())
            if h.hexdigest()[:16] == ent["kernel_source_sha16"]:
                res["roofline"]["traffic"] = ent["hbm_read_bytes_per_iteration"] + ent["hbm_write_bytes_per_iteration"]
                res["roofline"]["traffic_source"] = ent["source"]
            else:
                res["roofline"]["traffic_source"] = "stale: the loop kernels' sources changed since %s was captured" % ent["source"]
    except Exception:                                       # noqa: BLE001
        pass
    if survey_bytes is not None:      # what SURVEY section 8(d) counts for the reference's arithmetic on the same iteration (may exceed the peak: bytes never read)
        res["roofline"]["survey_8d_bytes_per_iteration"] = survey_bytes
        res["roofline"]["survey_8d_equivalent_GBps"] = survey_bytes / t_iter / 1e9
    res.update(extra)
    with open(out_path, "w") as f:
        json.dump(res, f)


def cpu_config_baseline(name, budget_s, seed):
    """cpu_baseline of one of the other configs (round 5: COMPILED): the C restatement of the reference's loop for that solver
    (oracle/c/admm_loops_cpu.c through oracle/cloops.py -- the checker of tests/test_oracle_cloops.py, here only TIMED) on the SAME
    shape, synthetic data of the same distribution, for as many iterations as fit `budget_s` (the loop cuts itself off), twice:
    ONE thread -- the reference's configuration (`Lasso.cpp:1` EIGEN_DONT_PARALLELIZE; R's reference BLAS for the dgemv of LAD / BP;
    only the consensus workers and the wide solver's active-set loop use OpenMP there) -- and all host threads, every product spread
    over them, pinned (`best_effort`; OMP_PROC_BIND / OMP_PLACES are set by main() before the library is loaded).  The one-time
    setup (Gram, factorisations: NumPy / LAPACK) is not part of either rate."""
    import numpy as np
    import torch
    os.environ.setdefault("OMP_PROC_BIND", "spread")       # (read when the OpenMP runtime starts: main() sets them first thing as well)
    os.environ.setdefault("OMP_PLACES", "cores")
    from oracle import cloops
    F = np.float32
    tg = torch.Generator(); tg.manual_seed(seed + 77)
    threads = cloops.max_threads()

    def randn(shape, dtype, sd=1.0):
        return (torch.randn(shape, generator=tg, dtype=dtype) * sd).numpy()

    scale = 1.0
    t_setup0 = time.time()
    if name == "c3":
        n, p = 2000, 200000
        X = np.asfortranarray(randn((p, n), torch.float32, 2.0).T)
        b = np.zeros(p, F); b[:100] = np.random.default_rng(seed).uniform(size=100)
        Y = (X[:, :100] @ b[:100] + randn((n,), torch.float32)).astype(F)
        X -= X.mean(axis=0, dtype=F)[None, :]
        X *= (1.0 / np.sqrt((X * X).sum(axis=0, dtype=F) / n)).astype(F)[None, :]
        Y = ((Y - Y.mean()) / Y.std()).astype(F)
        # (the constructor's n x n Gram -- 8e11 flop -- only serves the spectral-radius estimate: 30 power iterations of X (X'v) stand in,
        # setup is not timed)
        lambda0 = F(np.abs(X.T @ Y).max())
        v = np.ones(n, F) / np.sqrt(F(n))
        for _ in range(30):
            w = X @ (X.T @ v)
            nv = float(np.linalg.norm(w))
            v = (w / nv).astype(F)
        sprad = F(0.95 * nv)                                 # the reference's loose Lanczos value sits 3-8 % below lambda_max
        lam = np.float64(lambda0) * 0.01 ** (np.arange(100) / 99.0)
        what = f"ADMMBase::solve + ADMMLassoWide on n={n} p={p}, the automatic 100-lambda grid from a cold start until the budget is used"

        def run(nt, budget):
            _, niter, secs, _ = cloops.wide_loop(X, Y, sprad, lambda0, lam, -1.0, 1e-5, 1e-5, 10000, nthreads=nt, want_beta=False, budget_s=budget)
            return int(np.minimum(niter, 10000).sum()), secs
    elif name == "c4":
        # bounded sample: 2 of the 8 row blocks (2500 rows): the per-iteration cost is K workers x the same two products, so the
        # measured rate is scaled by 2 / 8 (said in `sample`); the all-core leg gives every worker half of the threads
        import scipy.linalg as sla
        n_full, K_full = 10000, 8
        n, p, K = 2500, 100000, 2
        X = randn((n, p), torch.float32, 2.0)
        b = np.zeros(p, F); b[:100] = np.random.default_rng(seed).uniform(size=100)
        Y = (X[:, :100] @ b[:100] + randn((n,), torch.float32)).astype(F)
        X -= X.mean(axis=0, dtype=F)[None, :]
        X *= (1.0 / np.sqrt((X * X).sum(axis=0, dtype=F) / n)).astype(F)[None, :]
        Y = ((Y - Y.mean()) / Y.std()).astype(F)
        lam0 = float(np.abs(X.T @ Y).max())
        rho = 0.55 * lam0 / K_full                           # PADMMLasso.h:199-200 with the full problem's K
        A = [np.asfortranarray(X[k * (n // K):(k + 1) * (n // K)]) for k in range(K)]
        del X
        Ab = [(a.T @ Y[k * (n // K):(k + 1) * (n // K)]).astype(F) for k, a in enumerate(A)]
        Lf = []
        for a in A:
            G = (a @ a.T).astype(F)
            G[np.arange(len(G)), np.arange(len(G))] += F(rho)
            Lf.append(np.tril(sla.cho_factor(G, lower=True, check_finite=False)[0]))
        scale = float(K) / K_full
        what = (f"PADMMBase_Master::solve with PADMMLasso workers (Woodbury branch, float LLT solve, 1250 x {p} blocks), lambda = 0.55 lambda_max; "
                f"SAMPLE: {K} of the {K_full} row blocks of n={n_full}, the measured rate scaled by {K}/{K_full}")

        def run(nt, budget):
            _, niter, secs = cloops.consensus_loop(A, Ab, Lf, p, [0.55 * lam0], rho, 1e-5, 1e-5, 10000, nthreads=nt, budget_s=budget)
            return int(np.minimum(niter, 10000).sum()), secs
    elif name == "c5lad":
        import scipy.linalg as sla
        n, p = 50000, 5000
        X = np.asfortranarray(randn((p, n), torch.float64, 2.0).T)
        Y = X @ np.random.default_rng(seed).uniform(size=p) + randn((n,), torch.float64)
        X /= np.sqrt((X * X).sum(axis=0) / n - X.mean(axis=0) ** 2)[None, :]
        Y = Y / Y.std()
        Lf = np.tril(sla.cho_factor(X.T @ X, lower=True, check_finite=False)[0])
        what = f"FADMMBase::solve + ADMMLAD (general branch X (X'X)^-1 X': two products with X and two triangular solves per iteration) on n={n} p={p}"

        def run(nt, budget):
            r = cloops.dense_loop(0, X, Lf, Y, 1.0, 1e-4, 1e-4, 10000, nthreads=nt, budget_s=budget)
            return min(int(r[4]), 10000), r[5]
    elif name == "c5bp":
        from oracle.solvers import BP
        n, p = 5000, 50000
        A = randn((n, p), torch.float64)
        bt = np.zeros(p); bt[np.random.default_rng(seed).choice(p, 500, replace=False)] = np.random.default_rng(seed + 1).uniform(size=500)
        s = BP(A, A @ bt, 1.0, 1e-4, 1e-4)
        B, c0 = np.asfortranarray(s.LinvA), s.cache_AAAb
        del s, A
        what = f"FADMMBase::solve + ADMMBP (two products with L^-1 A per iteration) on n={n} p={p}"

        def run(nt, budget):
            r = cloops.dense_loop(1, B, None, c0, 1.0, 1e-4, 1e-4, 10000, nthreads=nt, budget_s=budget)
            return min(int(r[4]), 10000), r[5]
    elif name == "c5parbp":
        n, p, N = 5000, 50000, 8
        A = randn((p, n), torch.float64).T                         # column-major n x p without a 2 GB copy
        bt = np.zeros(p); bt[np.random.default_rng(seed).choice(p, 500, replace=False)] = np.random.default_rng(seed + 1).uniform(size=500)
        bvec = A @ bt
        chunk = p // N
        sprad = []                                                  # the class's exact spectral norms (8 SVDs) replaced by 40 power iterations: setup only
        for i in range(N):
            Ai = A[:, i * chunk:(p if i == N - 1 else (i + 1) * chunk)]
            v = np.ones(Ai.shape[1]) / np.sqrt(Ai.shape[1])
            nv = 1.0
            for _ in range(40):
                w = Ai.T @ (Ai @ v)
                nv = float(np.linalg.norm(w))
                v = w / nv
            sprad.append(1.02 * nv)
        rho = 1.0 / float(np.mean(sprad))
        what = (f"the sharing-ADMM loop of TODO/PADMMBP.h as oracle/solvers.py SharingBP restates it (every column on every 10th iteration, the current "
                f"non-zeros otherwise), {N} column blocks, on n={n} p={p}")

        def run(nt, budget):
            _, niter, secs = cloops.sharing_loop(A, bvec, N, sprad, rho, 1e-4, 1e-4, 10000, nthreads=nt, budget_s=budget)
            return min(int(niter), 10000), secs
    else:
        return None
    t_setup = time.time() - t_setup0
    it1, s1 = run(1, budget_s)
    # all-core leg: the host may hand out fewer cores than it shows (cgroup quota on a shared box: 128 visible threads measured 4 x
    # one core on the tall loop): the same loop at all visible threads, 32 and 8, the best one reported with its thread count
    tried = []
    for nt in sorted({threads, min(threads, 32), min(threads, 8)}, reverse=True):
        if nt <= 1:
            continue
        itq, sq = run(nt, budget_s / 2)
        tried.append((itq / sq if sq > 0 else 0.0, nt, itq, sq))
    rate_n, threads, itn, sn = max(tried) if tried else (0.0, 1, 0, 0.0)
    tried_note = ", ".join("%d threads: %.3g it/s" % (nt, r * scale) for r, nt, _, _ in tried)
    it1, itn = it1 * scale, itn * scale
    return {"value": it1 / s1 if s1 > 0 else None, "unit": "iterations/s", "cores": 1, "kind": "port",
            "sample": f"compiled C restatement (oracle/c/admm_loops_cpu.c, gcc -O3 -fopenmp) of {what}; ONE thread: {it1:g} (scaled) iterations in {s1:.1f} s; "
                      f"data generation + setup (Gram / factorisation, NumPy) {t_setup:.1f} s not included",
            "best_effort": {"value": itn / sn if sn > 0 else None, "unit": "iterations/s", "cores": int(threads),
                            "sample": f"the same compiled loop with every product spread over {threads} OpenMP threads (OMP_PROC_BIND=spread, OMP_PLACES=cores): "
                                      f"{itn:g} (scaled) iterations in {sn:.1f} s; best of [{tried_note}]"}}


def run_side_measurement(a, rank, world, kind, backend, seconds, port_offset):
    """Run a child measurement (`kind` in {"consensus", "tallshard"}) in a separate process per rank, with its own
    rendezvous port and a time limit, so that a failure or a hang of a multi-process exchange path can never take the
    primary measurement down.  Returns a dict (rank 0) or None."""
    import subprocess
    import tempfile
    out_path = os.path.join(tempfile.gettempdir(), "admm_%s_%s_%s.json" % (kind, backend, os.environ.get("MASTER_PORT", "0")))
    if rank == 0 and os.path.exists(out_path):
        os.remove(out_path)
    env = dict(os.environ)
    multi = world > 1 or FORCE_DIST
    if multi:
        env["MASTER_ADDR"] = "127.0.0.1"
        env["MASTER_PORT"] = str(int(os.environ.get("MASTER_PORT", "29500")) + port_offset)
        # the children build their OWN rendezvous store on that port: do not let env:// look for torchrun's agent store there
        for k in [k for k in env if k.startswith("TORCHELASTIC_")]:
            env.pop(k)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "%s:%s:%s" % (kind, backend, out_path), "--seed", str(a.seed),
           "--n", str(a.n), "--p", str(a.p), "--m", str(a.m), "--nlambda", str(a.nlambda), "--steps", str(a.steps),
           "--warmup", str(a.warmup), "--profile-stride", str(a.profile_stride)] + (["--side-shapes", a.side_shapes] if a.side_shapes else [])
    try:
        r = subprocess.run(cmd, env=env, timeout=seconds, capture_output=True, text=True)
        if rank != 0:
            return None
        if r.returncode != 0 or not os.path.exists(out_path):
            return {"exchange": backend, "error": "%s child failed (rc=%d): %s" % (kind, r.returncode, (r.stderr or "")[-400:])}
        return json.load(open(out_path))
    except subprocess.TimeoutExpired:
        return {"exchange": backend, "error": "%s child exceeded %.0f s" % (kind, seconds)} if rank == 0 else None
    except Exception as e:                                  # noqa: BLE001
        return {"exchange": backend, "error": repr(e)} if rank == 0 else None


def main():
    a = parse()
    if a.child:
        kind, backend, out_path = a.child.split(":", 2)
        if kind == "config":
            config_child(a, backend, out_path)
            return
        {"consensus": consensus_child, "tallshard": tallshard_child, "widecols": widecols_child, "exchcheck": exchcheck_child}[kind](a, backend, out_path)
        return
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_spawn(a)
    # The JSON line must be the only thing on stdout: libraries loaded below (RCCL prints a version banner to stdout when
    # its first communicator is created, flushed at exit) get stderr as their fd 1; the line goes to the saved descriptor.
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != a.gpus:
        raise SystemExit(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={world}: refusing to run (the line would misreport n_gpus)")
    multi = world > 1 or FORCE_DIST
    import torch                      # before libadmm_hip: one HIP runtime per process
    import torch.distributed as dist
    ndev = torch.cuda.device_count()
    if OVERSUBSCRIBE:                 # test hook: several ranks per device, control plane over gloo (RCCL refuses two ranks on one device)
        local_rank = local_rank % max(1, ndev)
    elif local_rank >= ndev:
        raise SystemExit(f"bench.py: rank {rank} needs device {local_rank} but only {ndev} are visible")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if multi:
        if OVERSUBSCRIBE:
            dist.init_process_group(backend="gloo")
        else:
            dist.init_process_group(backend="nccl", device_id=dev)
        if dist.get_world_size() != a.gpus:
            raise SystemExit(f"bench.py: the process group holds {dist.get_world_size()} ranks, --gpus {a.gpus}")
    rdev = torch.device("cpu") if OVERSUBSCRIBE else dev      # where the control-plane reductions of this function live
    import numpy as np
    from admm_amd import admm_lasso, DevicePtr, LassoPlan, load, options
    lib = load()
    options.set(PROFILE_STRIDE=a.profile_stride)            # time every k-th x-update launch with HIP events (admm_hip_options.profile_stride)
    rc = lib.admm_hip_set_device(local_rank)
    assert rc == 0

    def barrier():
        if multi:
            dist.barrier()

    n, p = a.n, a.p
    # ---- synthetic data, generated in HBM.  xt is p x n row-major == X (n x p) column-major.
    g = torch.Generator(device=dev)
    g.manual_seed(a.seed + rank)
    xt = torch.empty((p, n), dtype=torch.float64, device=dev)
    chunk = max(1, (1 << 27) // n)
    for c0 in range(0, p, chunk):
        c1 = min(p, c0 + chunk)
        xt[c0:c1] = torch.randn((c1 - c0, n), generator=g, device=dev, dtype=torch.float64) * 2.0
    beta_true = torch.zeros(p, dtype=torch.float64, device=dev)
    beta_true[:a.m] = torch.rand(a.m, generator=g, device=dev, dtype=torch.float64)
    y = beta_true @ xt + torch.randn(n, generator=g, device=dev, dtype=torch.float64)
    torch.cuda.synchronize()

    # ---- one-time preparation (outside the timed region).  The first call of a process also pays the lazy loading of the
    # library's code objects and the first large allocations (what a fresh R session's first $fit() pays); with --full it is
    # done a second time for the steady-state cost (`setup_s`).
    model = admm_lasso(DevicePtr(xt.data_ptr()), DevicePtr(y.data_ptr()), n=n, p=p).penalty(nlambda=a.nlambda)
    t0 = time.time()
    plan = LassoPlan(model)
    lib.admm_hip_device_synchronize()
    setup_s_cold = time.time() - t0
    setup_s = None
    if a.full:
        plan.close()
        t0 = time.time()
        plan = LassoPlan(model)
        lib.admm_hip_device_synchronize()
        setup_s = time.time() - t0
    del xt
    torch.cuda.empty_cache()

    fit = None
    for _ in range(a.warmup):
        fit = plan.run()
    barrier()
    torch.cuda.synchronize()
    lib.admm_hip_device_synchronize()
    t0 = time.time()
    iters = 0
    xms, xsamp, loop_ms = 0.0, 0, 0.0
    for _ in range(a.steps):
        fit = plan.run()
        iters += int(fit.stats["total_iter"])
        xms += fit.stats["xupdate_ms_avg"] * fit.stats["xupdate_samples"]
        xsamp += int(fit.stats["xupdate_samples"])
        loop_ms += fit.stats["loop_ms_events"]
    torch.cuda.synchronize()
    lib.admm_hip_device_synchronize()
    barrier()
    elapsed = time.time() - t0
    if multi:
        t = torch.tensor([elapsed, float(iters)], dtype=torch.float64, device=rdev)
        tmax = t.clone()
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        tsum = t.clone()
        dist.all_reduce(tsum, op=dist.ReduceOp.SUM)
        elapsed_max, iters_all = float(tmax[0]), float(tsum[1])
    else:
        elapsed_max, iters_all = elapsed, float(iters)
    if a.dump_outputs and rank == 0:
        dump_outputs(fit, a.dump_outputs)

    # ---- side measurements in child processes (own rendezvous, time-limited): the paths with a real exchange step.  At N > 1 the
    # sharded run of the headline workload is the primary figure; everything else runs with --full only.
    consensus, shard = [], []
    exch = []
    backends = tuple(b for b in a.exchanges.split(",") if b in ("rccl", "peer"))
    if multi and a.full:
        for k, backend in enumerate(backends):
            exch.append(run_side_measurement(a, rank, world, "exchcheck", backend, 120.0, 5 + 6 * k))
            barrier()
        if rank == 0:
            good = [c["exchange"] for c in exch if c and c.get("all_ranks_correct")]
            for c in exch:
                if c and not c.get("all_ranks_correct"):
                    sys.stderr.write("[bench] exchange self-check over %s FAILED at %d ranks: %s -- the measurements over it are kept apart as `rejected` / `error`; "
                                     "continuing with %s\n" % (c["exchange"], world, c.get("error", "sums differ from the closed form (relative error %.2e)" % c.get("worst_relative_error_rank0", float("nan"))),
                                                                 ", ".join(good) if good else "the replica figure only"))
    if a.full and a.consensus_seconds > 0:
        for k, backend in enumerate(backends if multi else ("rccl",)):
            consensus.append(run_side_measurement(a, rank, world, "consensus", backend, a.consensus_seconds, 17 + 12 * k))
            barrier()
    widecols = []
    if multi and a.shard_seconds > 0:
        for k, backend in enumerate(backends):
            shard.append(run_side_measurement(a, rank, world, "tallshard", backend, a.shard_seconds, 41 + 12 * k))
            barrier()
        if a.full:
            for k, backend in enumerate(backends):
                widecols.append(run_side_measurement(a, rank, world, "widecols", backend, a.shard_seconds, 71 + 12 * k))
                barrier()
    cfg_results = {}
    if a.full and world == 1 and not FORCE_DIST and a.config_seconds > 0:
        # the headline plan's 400 MB inverse stays resident; the children need up to ~20 GB each (fp64 inputs + fp32 / fp64 copies)
        for k, name in enumerate(CONFIGS):
            cfg_results[name] = run_side_measurement(a, rank, world, "config", name, a.config_seconds, 101 + k)
    if rank == 0:
        x_ms = xms / max(1, xsamp)
        sym = int(fit.stats["xupdate_variant"]) == 1
        # algorithmic bytes of the x-update per launch: the cached inverse is symmetric, the
        # symmetric kernel needs its lower triangle once (2p^2 B); the full-matrix kernel reads 4p^2 B.
        alg_bytes = (2.0 if sym else 4.0) * p * p
        achieved = alg_bytes / (x_ms * 1e-3) if x_ms > 0 else 0.0
        kname = ("symv2_lower_kernel (x-update, lower triangle of the cached inverse x [u w])" if sym
                 else "gemv_t_kernel<float,2,4> (x-update, cached inverse x [u w])")
        traffic, traffic_src = None, None
        try:        # PMC counters cannot be collected from inside the run: quote the committed measurement for this exact shape,
            # and only while the kernel source it was taken from is unchanged (otherwise null: re-profile)
            import hashlib
            pmc = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
            ent = pmc.get("symv2_lower_kernel" if sym else "gemv_t_kernel")
            src = os.path.join(ROOT, "admm_amd", "csrc", "symv_kernels.h" if sym else "gemv_kernels.h")
            sha = hashlib.sha256(open(src, "rb").read()).hexdigest()[:16]
            if ent and int(ent["p"]) == p and ent.get("kernel_source_sha16") == sha:
                traffic = ent["hbm_read_bytes"] + ent["hbm_write_bytes"]
                traffic_src = ent["source"]
            elif ent:
                traffic_src = "stale: %s changed since %s was captured" % (os.path.basename(src), ent["source"])
        except Exception:
            pass
        out = {
            "metric": "ADMM iterations/sec, Lasso tall n=%d p=%d (100-lambda warm-started path)" % (n, p),
            "value": iters_all / elapsed_max,
            "unit": "iterations/s",
            "n_gpus": world,
            "steps": a.steps,
            "warmup": a.warmup,
            "ms_per_step": elapsed_max / a.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {"workload": "admm_lasso tall path (BASELINE configs[1])", "n": n, "p": p, "nlambda": a.nlambda,
                       "standardize": True, "intercept": True, "eps_abs": 1e-5, "eps_rel": 1e-5,
                       "parallelism": "replicas x%d" % world if world > 1 else "single GPU",
                       "iters_per_step": iters / a.steps, "step": "one cold-started warm-chained lambda path"},
            "setup_s_cold": setup_s_cold,
            "sec_to_eps_cold": setup_s_cold + elapsed / a.steps,
            "setup_breakdown_s": {k: fit.stats[k] for k in ("t_h2d", "t_standardize", "t_gram", "t_eigs", "t_factor")},
            "loop_ms_events_per_step": loop_ms / a.steps,
            "rho": fit.stats["rho"],
            "nnz_last_lambda": int(np.count_nonzero(fit.beta_dense[1:, -1])),
            "roofline": {"bound": "hbm", "kernel": kname,
                         "achieved": achieved / 1e9, "peak": HBM_PEAK / 1e9, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK, "traffic": traffic, "traffic_source": traffic_src,
                         "algorithmic_bytes_per_launch": alg_bytes, "avg_launch_ms": x_ms, "launches_timed": xsamp,
                         "survey_4p2_equivalent_GBps": 4.0 * p * p / (x_ms * 1e-3) / 1e9 if x_ms > 0 else 0.0},
        }
        if setup_s is not None:
            out["setup_s"] = setup_s
            out["sec_to_eps"] = setup_s + elapsed / a.steps
        consensus = [c for c in consensus if c]
        shard = [c for c in shard if c]
        if exch:
            out["exchange_self_check"] = [c for c in exch if c]
        if consensus:
            out["consensus"] = consensus[0] if len(consensus) == 1 else consensus
        widecols = [c for c in widecols if c]
        if widecols:
            out["wide_column_sharded"] = widecols
        if shard:
            out["sharded"] = shard
            ok = [c for c in shard if "error" not in c]
            # a sharded run only counts if its ranks agreed on every iteration count, every lambda converged, and -- for the
            # PEER exchange -- its total iteration count is the RCCL run's within 2 % (the two sum in different orders, so a few
            # stopping decisions may flip; a broken exchange does not stay that close)
            ref = next((c for c in ok if c["exchange"] == "rccl" and c.get("ranks_agree_on_niter") and c.get("all_lambdas_converged")), None)
            valid = []
            for c in ok:
                why = None
                if int(c.get("ranks_in_communicator", 0)) != world or int(c.get("n_gpus", 0)) != world:
                    why = "the communicator held %s ranks, not %d" % (c.get("ranks_in_communicator"), world)
                elif not c.get("ranks_agree_on_niter", True):
                    why = "ranks disagree on the iteration counts"
                elif not c.get("all_lambdas_converged", True):
                    why = "a lambda ran into maxit"
                elif ref is not None and abs(c["iterations_per_step"] - ref["iterations_per_step"]) > 0.02 * ref["iterations_per_step"]:
                    why = "iteration count deviates from the RCCL run by more than 2 %"
                if why:
                    c["rejected"] = why
                else:
                    valid.append(c)
            ok = valid
            if not ok:
                out["config"]["parallelism"] = "replicas x%d (no sharded run was valid: see `sharded`)" % world
            if ok:
                # N > 1: the primary line is the headline workload itself with its x-update spread over the N GPUs (total
                # work fixed: strong scaling), over the better of the two exchanges; the independent-replica figure
                # measured above moves to `replicas_weak`.
                best = max(ok, key=lambda c: c["iters_per_s"])
                out["replicas_weak"] = {"value": out["value"], "ms_per_step": out["ms_per_step"], "scaling": "weak",
                                        "note": "N independent replicas of the single-GPU solver (no exchange)"}
                out["value"] = best["iters_per_s"]
                out["ms_per_step"] = best["elapsed_s"] / best["steps"] * 1e3
                out["scaling"] = "strong"
                out["config"]["parallelism"] = "x-update sharded over %d GPUs, one all-reduce of 2p floats per iteration (%s)" % (world, best["exchange"])
                out["config"]["iters_per_step"] = best["iterations_per_step"]
                out["config"]["ranks_in_communicator"] = best["ranks_in_communicator"]
                out["setup_s"] = best["setup_s"]
                out["sec_to_eps"] = best["setup_s"] + best["elapsed_s"] / best["steps"]
                out["roofline"]["note"] = "single-GPU replica kernel; the sharded run's share is in `sharded`"
        if a.full and a.cpu_seconds > 0 and world == 1:     # the CPU leg is timed on rank 0 at N = 1 only
            try:
                out["cpu_baseline"] = cpu_baseline(p, a.nlambda, a.cpu_seconds, a.seed, n_full=n)
            except Exception as e:                          # noqa: BLE001 -- never lose the GPU line to the CPU leg
                out["cpu_baseline"] = {"value": None, "unit": "iterations/s", "cores": 0, "kind": "port", "sample": "failed: %r" % (e,)}
        if cfg_results:
            # every BASELINE config on one line: the headline first (its roofline / cpu_baseline are the top-level objects), then the
            # child runs, each with its own roofline and -- timed here on the host cores -- its own cpu_baseline
            cfgs = [{"workload": out["config"]["workload"], "value": out["value"], "unit": "iterations/s", "dtype": "f32", "n_gpus": 1,
                     "roofline": {k: out["roofline"][k] for k in ("bound", "achieved", "peak", "unit", "frac", "traffic")},
                     "cpu_baseline": {k: out.get("cpu_baseline", {}).get(k) for k in ("value", "unit", "cores", "kind")}, "see": "top level"}]
            for name, res in cfg_results.items():
                if not res:
                    continue
                if "error" in res:
                    cfgs.append(dict(CONFIGS[name], error=res["error"]))
                    continue
                res.pop("exchange", None)
                if a.cpu_config_seconds > 0:
                    try:
                        res["cpu_baseline"] = cpu_config_baseline(name, a.cpu_config_seconds, a.seed)
                        v = res["cpu_baseline"] and res["cpu_baseline"].get("value")
                        if v:
                            res["gpu_over_cpu_1core"] = res["value"] / v
                            be = res["cpu_baseline"]["best_effort"].get("value")
                            res["gpu_over_cpu_all_cores"] = res["value"] / be if be else None
                    except Exception as e:                  # noqa: BLE001 -- never lose the GPU numbers to a CPU leg
                        res["cpu_baseline"] = {"value": None, "unit": "iterations/s", "cores": 0, "kind": "port", "sample": "failed: %r" % (e,)}
                cfgs.append(res)
            out["configs"] = cfgs
        sys.stdout.flush()
        os.write(real_stdout, (json.dumps(out) + "\n").encode())
    plan.close()
    if multi:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
