"""Child process of tests/test_gpu_parallel_devices.py: plain admm_hip_parlasso / admm_hip_parbp_traced calls with the in-process
multi-device mode (option PAR_DEVICES) and without, results into an .npz.  A fresh process per case: the in-process ranks are
host threads of THIS process, and the parent must survive whatever happens here.

    python tests/par_devices_child.py <mode> <case> <out.npz>

modes: lasso (default | PAR_DEVICES=0 | PAR_DEVICES=0,0), bp (default | 0,0), fail (a rank fails on purpose on the host, then an
ordinary call), refuse (a process-wide SHM communicator is attached)."""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np


def lasso_call(lib, x, y, K, kw, devices):
    from admm_amd import admm_lasso, options
    from admm_amd._lib import last_parallel_layout
    m = admm_lasso(x, y).penalty(nlambda=kw["nlambda"]).opts(maxit=kw["maxit"])
    m.nthread = K
    _, head, tail, lam, beta, niter, stats, keep = m._common()
    with options(PAR_DEVICES=devices):
        t0 = time.time()
        rc = lib.admm_hip_parlasso(*head, K, *tail)
        dt = time.time() - t0
    err = lib.admm_hip_last_error().decode() if rc else ""
    return dict(rc=rc, err=err, lam=lam.copy(), beta=beta.copy(), niter=niter.copy(), layout=np.array(last_parallel_layout()), seconds=dt)


def main():
    mode, case, out = sys.argv[1], sys.argv[2], sys.argv[3]
    from admm_amd import _lib
    from dist_worker import problem
    lib = _lib.load()
    assert lib.admm_hip_set_device(0) == 0
    x, y, K, kw = problem(case)
    res = {}
    if mode == "lasso":
        for tag, dev in (("default", None), ("off", "0"), ("pair", "0,0")):
            r = lasso_call(lib, x, y, K, kw, dev)
            assert r["rc"] == 0, (tag, r["err"])
            for k, v in r.items():
                if k != "err":
                    res[f"{tag}_{k}"] = v
    elif mode == "bp":
        from admm_amd import admm_bp, options
        from admm_amd._lib import last_parallel_layout
        for tag, dev in (("default", None), ("pair", "0,0")):
            m = admm_bp(x, y).parallel(kw["nthread"], devices=dev)
            fit = m.fit(trace=True)
            res[f"{tag}_beta"] = fit.beta.toarray().ravel()
            res[f"{tag}_niter"] = np.array([fit.niter])
            res[f"{tag}_trace"] = fit.trace
            res[f"{tag}_layout"] = np.array(last_parallel_layout())
            res[f"{tag}_exchange_variant"] = np.array([fit.stats["exchange_variant"]])
    elif mode == "fail":
        from admm_amd import options
        r = lasso_call(lib, x, y, K, kw, None)
        assert r["rc"] == 0, r["err"]
        for k in ("lam", "beta", "niter"):
            res[f"before_{k}"] = r[k]
        with options(TEST_PAR_FAIL_RANK="1"):
            r = lasso_call(lib, x, y, K, kw, "0,0")
        res["fail_rc"], res["fail_seconds"] = np.array([r["rc"]]), np.array([r["seconds"]])
        print("failing call:", r["rc"], r["err"], f"{r['seconds']:.2f} s", flush=True)
        for tag, dev in (("after", "0,0"), ("default", None)):
            r = lasso_call(lib, x, y, K, kw, dev)
            assert r["rc"] == 0, (tag, r["err"])
            for k in ("lam", "beta", "niter", "layout"):
                res[f"{tag}_{k}"] = r[k]
    elif mode == "refuse":
        from admm_amd import dist as adist
        adist.init_comm_shm(1, 0, "/admm_hip_pardev_" + str(os.getpid()), int.from_bytes(os.urandom(7), "little") | 1)
        r = lasso_call(lib, x, y, K, kw, "0,0")
        res["refuse_rc"] = np.array([r["rc"]])
        print("refused:", r["rc"], r["err"], flush=True)
        adist.finalize_comm()
    else:
        raise SystemExit("unknown mode " + mode)
    np.savez(out, **res)
    print("ok", flush=True)


if __name__ == "__main__":
    main()
