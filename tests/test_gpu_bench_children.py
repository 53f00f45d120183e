"""GPU, two PROCESSES on one device: bench.py's multi-rank children -- the code the driver's `--gpus N` run executes and nothing
else in the suite did (round-3 review: "the first 8-GPU driver run would be the first execution of that code with N > 1").

Each child kind (`tallshard`: the headline workload with its x-update spread over the ranks; `widecols`: the column-sharded wide
solver; `consensus`: BASELINE configs[3] with its 8 row blocks spread over the ranks) is launched exactly as
bench.run_side_measurement launches it -- `python bench.py --child kind:backend:out.json`, one process per rank, its own gloo
rendezvous -- as two ranks on ONE GPU over the PEER (hipIpc-mapped exchange slots) and the SHM back-ends (RCCL refuses two ranks
on one device), at reduced shapes.  Asserted: every rank exits 0, the ranks agree on every iteration count, every lambda
converged, and the PEER and SHM runs (bit-identical exchanges by construction) took identical iteration totals -- the acceptance
rules bench.py itself applies to a sharded result (`ranks_agree_on_niter`, convergence, iteration total within 2 % of the
reference exchange)."""
import json
import os
import socket
import subprocess
import sys
import tempfile

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_child(kind, backend, nranks=2, timeout=420):
    with tempfile.TemporaryDirectory(prefix="admmbench") as wd:
        out = os.path.join(wd, "out.json")
        port = _free_port()
        procs = []
        for r in range(nranks):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK="0", WORLD_SIZE=str(nranks), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                       HSA_ENABLE_IPC_MODE_LEGACY="0")
            cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--child", f"{kind}:{backend}:{out}", "--n", "24000", "--p", "2304", "--m", "100",
                   "--nlambda", "12", "--steps", "1", "--warmup", "1", "--side-shapes", "2000,20000;600,30000,8"]
            procs.append(subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        outs = []
        try:
            for pr in procs:
                o, _ = pr.communicate(timeout=timeout)
                outs.append(o)
        finally:
            for pr in procs:
                if pr.poll() is None:
                    pr.kill()
        for r, pr in enumerate(procs):
            assert pr.returncode == 0, f"{kind} over {backend}: rank {r} failed:\n{outs[r][-3000:]}"
        return json.load(open(out))


@pytest.mark.parametrize("kind", ["tallshard", "widecols", "consensus"])
def test_bench_multi_rank_child_as_two_processes(kind):
    res = {b: _run_child(kind, b) for b in ("peer", "shm")}
    for b, r in res.items():
        assert "error" not in r, (kind, b, r)
        assert r["n_gpus"] == 2 and r["ranks_in_communicator"] == 2 and r["exchange"] == b
        assert r["ranks_agree_on_niter"] is True, (kind, b, r)
        assert r.get("all_lambdas_converged", r.get("converged")) is True, (kind, b, r)
        assert r["iters_per_s"] > 0
    it = {b: r.get("iterations", r.get("iterations_per_step")) for b, r in res.items()}
    assert it["peer"] == it["shm"], (kind, it)                       # the two exchanges add in the same order: identical decisions
    if kind == "consensus":
        assert res["peer"]["K"] == 8 and res["peer"]["scaling"] == "strong"
    print(f"[bench child {kind}] 2 ranks on one GPU: " + ", ".join(f"{b}: {it[b]} iterations, {res[b]['iters_per_s']:.0f} it/s" for b in res))


def test_bench_exchange_self_check_as_two_processes():
    """bench.py's first step at N > 1 (exchcheck_child): the all-reduce of each back-end against the closed-form sum, two ranks on one GPU
    over PEER and SHM -- the child that tells the first multi-GPU run WHICH exchange works there."""
    for b in ("peer", "shm"):
        r = _run_child("exchcheck", b, timeout=180)
        assert r["exchange"] == b and r["ranks"] == 2 and r["all_ranks_correct"] is True, r
        assert r["worst_relative_error_rank0"] < 1e-6, r


def test_bench_gpus2_without_a_launcher_spawns_its_ranks():
    """`python bench.py --gpus 2` started WITHOUT torchrun and without WORLD_SIZE (round-5 review: it ran one GPU and printed n_gpus: 1):
    it must re-execute itself under torch.distributed.run with two ranks and print a line that says n_gpus: 2, whose primary figure
    comes from a sharded run whose communicator really held two ranks (admm_hip_comm_info).  One-GPU box: the two ranks share the
    device (ADMM_BENCH_OVERSUBSCRIBE=1: local_rank modulo the device count, control plane over gloo) and only the PEER exchange runs
    (RCCL refuses two ranks on one device)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(ADMM_BENCH_OVERSUBSCRIBE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--n", "24000", "--p", "2304", "--m", "100", "--nlambda", "12", "--steps", "1",
           "--warmup", "1", "--full", "--exchanges", "peer", "--consensus-seconds", "0", "--shard-seconds", "240", "--cpu-seconds", "0",
           "--side-shapes", "2000,20000;600,30000,8"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2, out
    assert out["scaling"] == "strong" and out["config"]["ranks_in_communicator"] == 2, out["config"]
    sh = [c for c in out["sharded"] if "error" not in c]
    assert sh and all(c["ranks_in_communicator"] == 2 and c["n_gpus"] == 2 and "rejected" not in c for c in sh), out["sharded"]
    assert out["replicas_weak"]["value"] > 0
    assert [c for c in out["exchange_self_check"] if c["exchange"] == "peer"][0]["all_ranks_correct"] is True
    print(f"[bench --gpus 2, self-spawned] {out['value']:.0f} it/s sharded over 2 ranks ({out['config']['parallelism']}); replicas {out['replicas_weak']['value']:.0f} it/s")


def test_bench_refuses_a_world_size_that_disagrees_with_gpus():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "1"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "refusing" in (r.stderr + r.stdout), (r.returncode, r.stderr[-500:])
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
