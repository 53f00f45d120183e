"""The gate of the packed x-update stream: the bare one-vector tile loop on the fp32 inverse against the same loop on its exact 29-bit
copy (admm_hip_test_symv_packed_time), event-timed launch by launch, on cold caches and replayed back to back.

    python scripts/symv_packed_gate.py [--p 10000] [--reps 20] [--out FILE.json]

The matrix is inverse-like (unit diagonal, off-diagonals 3e-3 N(0, 1)); the timing does not depend on the values beyond the escape count."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--p", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from admm_amd import _lib
    fp = ctypes.POINTER(ctypes.c_float)
    rng = np.random.default_rng(a.p)
    A = np.empty((a.p, a.p), dtype=np.float32, order="F")
    for j0 in range(0, a.p, 1000):                      # in column panels: no second 400 MB temporary
        A[:, j0:j0 + 1000] = 3e-3 * rng.standard_normal((a.p, min(1000, a.p - j0)), dtype=np.float32)
    A[np.diag_indices(a.p)] = 1.0                       # (only the lower triangle is read)
    v = rng.standard_normal(a.p).astype(np.float32)
    us = np.zeros((4, a.reps), np.float32)
    info = (ctypes.c_longlong * 4)()
    _lib.check(_lib.load().admm_hip_test_symv_packed_time(A.ctypes.data_as(fp), a.p, v.ctypes.data_as(fp), a.reps, us.ctypes.data_as(fp), info))
    names = ["fp32 cold", "packed cold", "fp32 back to back", "packed back to back"]
    res = {"p": a.p, "reps": a.reps, "tiles": int(info[0]), "escapes": int(info[1]), "tiles_overflowed": int(info[2]), "packed_bytes": int(info[3]),
           "fp32_bytes": 2 * a.p * a.p}
    for k, n in enumerate(names):
        r = us[k]
        res[n] = {"min": float(r.min()), "median": float(np.median(r)), "mean": float(r.mean()), "max": float(r.max()), "all": [round(float(x), 2) for x in r]}
        print("%-22s min %7.2f  median %7.2f  mean %7.2f  max %7.2f us" % (n, r.min(), np.median(r), r.mean(), r.max()))
    print(json.dumps({k: v for k, v in res.items() if not isinstance(v, dict)}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
