"""The gate of the packed x-update stream: the bare one-vector tile loop on the fp32 inverse against the same loop on its exact 29-bit
copy (admm_hip_test_symv_packed_time), event-timed launch by launch, on cold caches and replayed back to back.

    python scripts/symv_packed_gate.py [--p 10000] [--reps 20] [--out FILE.json] [--against NAME=LIB.so ...] [--rounds 3]

The matrix is inverse-like (unit diagonal, off-diagonals 3e-3 N(0, 1)); the timing does not depend on the values beyond the escape count.

--against: other builds of the same library -- the parent commit's, or a dev flavour of the packed loop (ADMM_HIP_EXTRA_CXXFLAGS with
-DADMM_HIP_SYMV1_DEPTH=1, -DADMM_HIP_SYMV1_WGS=5, ... and `python -m admm_amd.build`, the library copied aside) -- timed in this same
process on the same matrix: `rounds` rounds, and within a round every build once, one after the other, so that no build has the device
to itself earlier or later than the others."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NAMES = ["fp32 cold", "packed cold", "fp32 back to back", "packed back to back"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--p", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--against", action="append", default=[], metavar="NAME=LIB")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    from admm_amd import _lib
    fp = ctypes.POINTER(ctypes.c_float)
    builds = [("tree", _lib.load())]
    for spec in a.against:
        name, _, path = spec.partition("=")
        other = ctypes.CDLL(os.path.abspath(path))
        other.admm_hip_test_symv_packed_time.argtypes = builds[0][1].admm_hip_test_symv_packed_time.argtypes
        other.admm_hip_test_symv_packed_time.restype = ctypes.c_int
        builds.append((name, other))
    rounds = a.rounds if len(builds) > 1 else 1
    rng = np.random.default_rng(a.p)
    A = np.empty((a.p, a.p), dtype=np.float32, order="F")
    for j0 in range(0, a.p, 1000):                      # in column panels: no second 400 MB temporary
        A[:, j0:j0 + 1000] = 3e-3 * rng.standard_normal((a.p, min(1000, a.p - j0)), dtype=np.float32)
    A[np.diag_indices(a.p)] = 1.0                       # (only the lower triangle is read)
    v = rng.standard_normal(a.p).astype(np.float32)
    res = {"p": a.p, "reps": a.reps, "rounds": rounds, "fp32_bytes": 2 * a.p * a.p, "builds": {}}
    us = {name: np.zeros((4, rounds * a.reps), np.float32) for name, _ in builds}
    for rnd in range(rounds):
        for name, lib in builds:
            one = np.zeros((4, a.reps), np.float32)
            info = (ctypes.c_longlong * 4)()
            code = lib.admm_hip_test_symv_packed_time(A.ctypes.data_as(fp), a.p, v.ctypes.data_as(fp), a.reps, one.ctypes.data_as(fp), info)
            if code != 0:
                raise RuntimeError("admm_hip_test_symv_packed_time failed in build %r with code %d" % (name, code))
            us[name][:, rnd * a.reps:(rnd + 1) * a.reps] = one
            res.update({"tiles": int(info[0]), "escapes": int(info[1]), "tiles_overflowed": int(info[2]), "packed_bytes": int(info[3])})
    for name, _ in builds:
        res["builds"][name] = {}
        for k, n in enumerate(NAMES):
            r = us[name][k]
            per_round = [float(np.median(r[i * a.reps:(i + 1) * a.reps])) for i in range(rounds)]
            res["builds"][name][n] = {"min": float(r.min()), "median": float(np.median(r)), "mean": float(r.mean()), "max": float(r.max()),
                                      "median_per_round": [round(x, 2) for x in per_round], "all": [round(float(x), 2) for x in r]}
            print("%-10s %-22s min %7.2f  median %7.2f  mean %7.2f  max %7.2f us   per round %s"
                  % (name, n, r.min(), np.median(r), r.mean(), r.max(), " ".join("%.2f" % x for x in per_round)))
    print(json.dumps({k: v for k, v in res.items() if not isinstance(v, dict)}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
