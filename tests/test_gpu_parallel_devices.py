"""GPU: the in-process multi-device mode of admm_hip_parlasso / admm_hip_parbp (option PAR_DEVICES).  On one GPU the test form
PAR_DEVICES=0,0 runs two ranks as two host threads of ONE process on device 0, over the in-process PEER communicator.  Same kernels
and same rank-order sums as two processes over the PEER backend (tests/test_gpu_dist2.py), so the results must be bit-identical to
that run.  Every case runs in a fresh child process (tests/par_devices_child.py) under a time limit, with GPU_MAX_HW_QUEUES=8 so
that each rank's stream has a hardware queue of its own."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _child(mode, case, timeout=300):
    with tempfile.TemporaryDirectory(prefix="admmpardev") as wd:
        out = os.path.join(wd, "out.npz")
        env = dict(os.environ, GPU_MAX_HW_QUEUES="8")
        pr = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, os.path.join(HERE, "par_devices_child.py"), mode, case, out],
                            env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert pr.returncode == 0, f"child {mode} {case} failed ({pr.returncode}):\n{pr.stdout[-3000:]}"
        return dict(np.load(out)), pr.stdout


def _two_process_peer(case):
    with tempfile.TemporaryDirectory(prefix="admmdist") as wd:
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs = [subprocess.Popen(["timeout", "-k", "10", "300", sys.executable, os.path.join(HERE, "dist_worker.py"), "peer", str(r), "2", wd, case],
                                  env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
        outs = [pr.communicate()[0] for pr in procs]
        for r, pr in enumerate(procs):
            assert pr.returncode == 0, f"rank {r} failed:\n{outs[r][-3000:]}"
        return [dict(np.load(os.path.join(wd, f"result.{r}.npz"))) for r in range(2)]


@pytest.mark.parametrize("case", ["tallblocks", "wideblocks", "wideblocks_k2"])
def test_parlasso_two_ranks_in_process_matches_two_processes(case):
    res, _ = _child("lasso", case)
    assert list(res["pair_layout"]) == [0, 0]                      # really ran as two ranks
    assert list(res["default_layout"]) == [0] and list(res["off_layout"]) == [0]
    # option unset and PAR_DEVICES=0: the single-device path, byte for byte
    for k in ("lam", "beta", "niter"):
        assert np.array_equal(res[f"default_{k}"], res[f"off_{k}"]), k
    two = _two_process_peer(case)
    assert np.array_equal(res["pair_lam"], two[0]["lam"])
    assert np.array_equal(res["pair_niter"], two[0]["niter"])
    assert np.array_equal(res["pair_beta"], two[0]["beta"]), float(np.abs(res["pair_beta"] - two[0]["beta"]).max())


def test_parbp_two_ranks_in_process_matches_two_processes():
    sys.path.insert(0, HERE)
    from dist_worker import problem
    res, _ = _child("bp", "parbp")
    assert list(res["pair_layout"]) == [0, 0] and list(res["default_layout"]) == [0]
    assert int(res["pair_exchange_variant"][0]) == 1 and int(res["default_exchange_variant"][0]) == 0
    two = _two_process_peer("parbp")
    x, y, _, kw = problem("parbp")
    beta2 = np.zeros(x.shape[1])
    for r in range(2):
        lo, hi = two[r]["lo"]
        beta2[lo:hi] = two[r]["beta"]
        assert int(two[r]["niter"][0]) == int(res["pair_niter"][0])
    assert np.array_equal(res["pair_beta"], beta2), float(np.abs(res["pair_beta"] - beta2).max())
    # the decision trace of rank 0 (replicated decisions) is that of a complete solve
    assert len(res["pair_trace"]) > 0


def test_failing_rank_ends_the_call_and_the_next_call_works():
    res, out = _child("fail", "tallblocks", timeout=120)
    rc = int(res["fail_rc"][0])
    assert rc in (7, 8), out                                        # ADMM_ERR_COMM or the injected ADMM_ERR_INTERNAL
    assert float(res["fail_seconds"][0]) < 10.0, out
    assert list(res["after_layout"]) == [0, 0] and list(res["default_layout"]) == [0]
    # the ordinary call after the failure: byte-identical to the same call before it
    for k in ("lam", "beta", "niter"):
        assert np.array_equal(res[f"default_{k}"], res[f"before_{k}"]), k


def test_refused_while_a_process_wide_communicator_is_attached():
    res, out = _child("refuse", "tallblocks", timeout=120)
    assert int(res["refuse_rc"][0]) == 1, out                       # ADMM_ERR_INVALID_ARG
    assert "process-wide communicator" in out
