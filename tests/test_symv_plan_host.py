"""The host half of the tall x-update's plan (symv_plan_layout, symv_kernels.h) through admm_hip_test_symv_plan, without a GPU: every
pair of segment widths the option parser accepts, every split, ragged and aligned orders, and the lists dealt out to the ranks of the
row-sharded solver.  Everything is asserted from the returned tiles: their shape, that the tiles of a strip partition its columns,
that the parts partition the whole list, and that every partial slot the consumer (symv_sum_partials) reads is written by exactly one
tile.  All tile boundaries are multiples of 32 columns and of 256 rows, so the slot counts are taken per 32-column unit of the dot
rows and per 256-row strip of the axpy rows: that is exact, not a sample.

Also here: the four hooks of tests/test_gpu_symv_variants.py refuse bad requests before they look for a device."""
import ctypes
import os

import numpy as np
import pytest

INVALID_ARG, NO_DEVICE = 1, 2
CAP = 1 << 15
WIDTHS = tuple(range(32, 257, 32))
SPLITS = (0, 250, 500, 750, 1000)
ORDERS = (3, 31, 32, 33, 255, 256, 257, 260, 383, 385, 513, 769, 1025, 1100, 2049, 2303, 4200, 6000, 10000)
NPARTS = (2, 3, 4, 8)
_ip = ctypes.POINTER(ctypes.c_int)
_fp = ctypes.POINTER(ctypes.c_float)
_dp = ctypes.POINTER(ctypes.c_double)


def _L():
    from admm_amd import _lib
    return _lib


_tiles_buf = np.empty((CAP, 4), dtype=np.int32)


def _plan(p, part=0, nparts=1, cus=256):
    """(sched, info, tiles): tiles an int64 copy [ntiles][4] of (rb, c0, width, seg)."""
    L = _L()
    sched = (ctypes.c_int * 3)()
    info = (ctypes.c_longlong * 6)()
    L.check(L.load().admm_hip_test_symv_plan(p, cus, part, nparts, sched, info, _tiles_buf.ctypes.data_as(_ip), CAP))
    keys = ("nrb", "p32", "ldo", "nax_rows", "nt", "ntiles")
    info = dict(zip(keys, (int(v) for v in info)))
    return tuple(sched), info, _tiles_buf[:info["ntiles"]].astype(np.int64)


def _key(t):
    return t[:, 0] * (1 << 20) + t[:, 1]          # (rb, c0) names a tile


def _check_full_list(p, sched, info, t):
    wb, ws, split = sched
    nrb, p32, ldo = info["nrb"], info["p32"], info["ldo"]
    assert nrb == -(-p // 256) and p32 == -(-p // 32) * 32 and ldo == nrb * 256 and info["ntiles"] == len(t) > 0
    rb, c0, w, seg = t.T
    strip_w = np.where(rb >= split, wb, ws)                                 # SymvSched::width
    cols = np.minimum((rb + 1) * 256, p32)
    # tile shape
    assert ((w > 0) & (w % 32 == 0) & (w <= 256)).all()
    assert ((rb >= 0) & (rb < nrb) & (seg >= 0)).all()
    assert (c0 == seg * strip_w).all()
    assert (c0 + w <= cols).all()
    # partition: sorted by (rb, c0), every strip starts at 0, goes on without gap or overlap and ends at its last column
    o = np.lexsort((c0, rb))
    rb_s, c0_s, end_s, seg_s = rb[o], c0[o], (c0 + w)[o], seg[o]
    first = np.r_[True, rb_s[1:] != rb_s[:-1]]
    last = np.r_[first[1:], True]
    assert np.array_equal(rb_s[first], np.arange(nrb))                      # every strip is there
    assert (c0_s[first] == 0).all() and (end_s[last] == np.minimum((rb_s[last] + 1) * 256, p32)).all()
    assert (c0_s[1:][~first[1:]] == end_s[:-1][~first[1:]]).all()
    nseg_strip = np.bincount(rb_s, minlength=nrb)
    assert (seg_s == np.arange(len(t)) - np.repeat(np.flatnonzero(first), nseg_strip)).all()   # seg = index within the strip
    assert info["nax_rows"] == nseg_strip.max()
    # launch order: long strips first
    assert (np.diff(rb) <= 0).all()
    # consumer slots, dot rows: counts per 32-column unit
    nu = ldo // 32
    reps = w // 32
    start = rb * nu + c0 // 32
    unit = np.repeat(start, reps) + (np.arange(reps.sum()) - np.repeat(np.cumsum(reps) - reps, reps))
    dot_written = np.bincount(unit, minlength=nrb * nu).reshape(nrb, nu)
    u = np.arange(nu)
    dot_read = (np.arange(nrb)[:, None] >= (u // 8)[None, :]) & (u * 32 < p)[None, :]      # dot[rb][i], rb = i / 256 .. nrb - 1, i < p
    assert (dot_written[dot_read] == 1).all() and dot_written.max() <= 1
    # consumer slots, axpy rows: counts per 256-row strip; the consumer reads s < SymvSched::nseg(i / 256, p32)
    width_of = np.where(np.arange(nrb) >= split, wb, ws)
    nseg_consumer = -(-np.minimum((np.arange(nrb) + 1) * 256, p32) // width_of)
    axp_written = np.bincount(seg * nrb + rb, minlength=info["nax_rows"] * nrb).reshape(info["nax_rows"], nrb)
    axp_read = np.arange(info["nax_rows"])[:, None] < nseg_consumer[None, :]
    assert nseg_consumer.max() <= info["nax_rows"]
    assert (axp_written[axp_read] == 1).all() and axp_written.max() <= 1


def _check_parts(p, full_sched, full_tiles, cus=256):
    full_keys = np.sort(_key(full_tiles))
    for nparts in NPARTS:
        got = []
        for part in range(nparts):
            sched, info, t = _plan(p, part, nparts, cus)
            assert sched == full_sched
            got.append(t)
        allt = np.concatenate(got)
        keys = _key(allt)
        o = np.argsort(keys, kind="stable")
        assert np.array_equal(keys[o], full_keys), (p, nparts)              # pairwise disjoint, and the union is the whole list
        fo = np.argsort(_key(full_tiles), kind="stable")
        assert np.array_equal(allt[o], full_tiles[fo])                      # ... with every record as it was


@pytest.mark.parametrize("wb", WIDTHS)
def test_every_width_pair_split_and_order(wb):
    """8 x 8 width pairs (one width_big per case) x 5 splits x 19 orders x nparts 1, 2, 3, 4, 8 with every part."""
    L = _L()
    for ws in WIDTHS:
        for split in SPLITS:
            with L.options(SYMV_SCHED="%d,%d,%d" % (wb, ws, split)):
                for p in ORDERS:
                    sched, info, t = _plan(p)
                    assert sched == (wb, ws, split * info["nrb"] // 1000), (p, sched)
                    _check_full_list(p, sched, info, t)
                    _check_parts(p, sched, t)


def test_default_schedules_at_256_compute_units():
    """The classes the comment in symv_plan_layout documents, and a CU count <= 0 means 256."""
    want = {2048: (32, 32), 3000: (32, 32), 4096: (64, 64), 6000: (128, 64), 8000: (128, 64), 10000: (192, 64), 16000: (192, 64)}
    for p, (wb, ws) in want.items():
        for cus in (256, 0, -1):
            sched, info, t = _plan(p, cus=cus)
            assert sched == (wb, ws, 0 if wb == ws else info["nrb"] // 2), (p, cus, sched)
        _check_full_list(p, sched, info, t)
    assert _plan(12449)[1]["nt"] == 0 and _plan(12451)[1]["nt"] == 1        # 2 p^2 bytes against 310 MB
    assert _plan(16000, 0, 2)[1]["nt"] == 0 and _plan(20000, 1, 2)[1]["nt"] == 1


@pytest.mark.parametrize("cus", [256, 64, 8])
def test_default_schedule_dealt_out(cus):
    """Without an override the schedule depends on nparts (a rank launches 1 / nparts of the tiles), so the whole list to compare with
    is the one of an override with the values the hook reports: rb_split = nrb / 2 is 500 per mille, 0 is 0."""
    L = _L()
    seen = set()
    for p in ORDERS + (8000, 16000):
        for nparts in NPARTS:
            parts = [_plan(p, part, nparts, cus) for part in range(nparts)]
            sched = parts[0][0]
            assert all(q[0] == sched for q in parts)
            nrb = parts[0][1]["nrb"]
            assert sched[2] == (0 if sched[0] == sched[1] else nrb // 2)
            seen.add(sched[:2])
            with L.options(SYMV_SCHED="%d,%d,%d" % (sched[0], sched[1], 0 if sched[2] == 0 else 500)):
                fsched, finfo, full = _plan(p, cus=cus)
            assert fsched == sched
            allt = np.concatenate([q[2] for q in parts])
            o = np.argsort(_key(allt), kind="stable")
            assert np.array_equal(allt[o], full[np.argsort(_key(full), kind="stable")]), (p, nparts, cus)
    assert len(seen) >= 2                                                    # more than one class was dealt out


# ---- the conventions of the hooks (as tests/test_factor_hooks_host.py)

def _args(p=5):
    A = np.eye(p, dtype=np.float32, order="F")
    v = np.ones(p, dtype=np.float32)
    V = np.ones((2, p), dtype=np.float32)
    y0, y1 = np.zeros(p, np.float32), np.zeros(p, np.float32)
    d0, d1 = np.zeros(p), np.zeros(p)
    Y = np.zeros((2, p), np.float32)
    return dict(A=A.ctypes.data_as(_fp), v0=v.ctypes.data_as(_fp), v1=v.ctypes.data_as(_fp), V=V.ctypes.data_as(_fp), y0=y0.ctypes.data_as(_fp),
                y1=y1.ctypes.data_as(_fp), d0=d0.ctypes.data_as(_dp), d1=d1.ctypes.data_as(_dp), Y=Y.ctypes.data_as(_fp), sched=(ctypes.c_int * 3)(),
                keep=(A, v, V, y0, y1, d0, d1, Y))


def _ex(lib, a, p=5, variant=0, part=0, nparts=1, **ptr):
    g = dict(a, **ptr)
    return lib.admm_hip_test_symv_ex(g["A"], p, g["v0"], g["v1"], variant, part, nparts, g["y0"], g["y1"], g["sched"])


def _multi(lib, a, p=5, nr=2, rhs=2, nt=0, finish=0, **ptr):
    g = dict(a, **ptr)
    return lib.admm_hip_test_symv_multi_ex(g["A"], p, g["V"], nr, rhs, nt, finish, g["Y"], g["sched"])


def _f64(lib, a, p=5, **ptr):
    g = dict(a, **ptr)
    return lib.admm_hip_test_symv_f64acc(g["A"], p, g["v0"], g["v1"], g["d0"], g["d1"], g["sched"])


def test_hooks_refuse_bad_arguments_before_they_look_for_a_device():
    lib = _L().load()
    a = _args()
    sched, info = (ctypes.c_int * 3)(), (ctypes.c_longlong * 6)()
    tiles = (ctypes.c_int * 64)()
    plan_bad = [(0, 256, 0, 1, sched, info, tiles, 16), (32769, 256, 0, 1, sched, info, tiles, 16), (5, 256, 1, 1, sched, info, tiles, 16),
                (5, 256, -1, 2, sched, info, tiles, 16), (5, 256, 0, 0, sched, info, tiles, 16), (5, 256, 0, 65, sched, info, tiles, 16),
                (5, 256, 0, 1, None, info, tiles, 16), (5, 256, 0, 1, sched, None, tiles, 16), (5, 256, 0, 1, sched, info, None, 16),
                (5, 256, 0, 1, sched, info, tiles, 0), (5, 1 << 20, 0, 1, sched, info, tiles, 16)]
    for args in plan_bad:
        assert lib.admm_hip_test_symv_plan(*args) == INVALID_ARG, args[:4]
        assert "symv plan hook" in lib.admm_hip_last_error().decode()
    info[5] = -7
    assert lib.admm_hip_test_symv_plan(2049, 256, 0, 1, sched, info, tiles, 16) == INVALID_ARG      # 9 x 8 + ... tiles do not fit 16 records
    assert "tile_capacity" in lib.admm_hip_last_error().decode() and info[5] == -7                  # and nothing was written
    for call, bad in ((_ex, [dict(A=None), dict(v0=None), dict(v1=None), dict(y0=None), dict(y1=None), dict(sched=None), dict(p=0), dict(p=32769),
                             dict(variant=-1), dict(variant=3), dict(nparts=0), dict(nparts=65), dict(part=1), dict(part=-1, nparts=2), dict(part=2, nparts=2)]),
                      (_multi, [dict(A=None), dict(V=None), dict(Y=None), dict(sched=None), dict(p=0), dict(p=32769), dict(nr=0), dict(nr=65), dict(rhs=3),
                                dict(rhs=0), dict(rhs=16), dict(nt=2), dict(nt=-1), dict(finish=2), dict(finish=-1)]),
                      (_f64, [dict(A=None), dict(v0=None), dict(v1=None), dict(d0=None), dict(d1=None), dict(sched=None), dict(p=0), dict(p=32769)])):
        for spoil in bad:
            assert call(lib, a, **spoil) == INVALID_ARG, (call.__name__, spoil)
            assert "hook" in lib.admm_hip_last_error().decode()


def test_symbols_are_declared_exported_bound_and_listed():
    import re
    L = _L()
    lib = L.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "admm_hip.h")).read(), flags=re.S)
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    for sym in ("admm_hip_test_symv_plan", "admm_hip_test_symv_ex", "admm_hip_test_symv_multi_ex", "admm_hip_test_symv_f64acc"):
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
        assert hasattr(lib, sym) and sym in L.EXPORTS
        assert getattr(lib, sym).argtypes is not None and getattr(lib, sym).restype is ctypes.c_int
        assert "`%s`" % sym in doc, sym


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful on a machine without a GPU")
def test_valid_requests_find_no_device_and_the_plan_hook_needs_none():
    lib = _L().load()
    a = _args()
    assert _ex(lib, a) == NO_DEVICE and _ex(lib, a, variant=2, part=1, nparts=3) == NO_DEVICE
    assert _multi(lib, a) == NO_DEVICE and _multi(lib, a, nr=1, rhs=12, nt=1, finish=1) == NO_DEVICE
    assert _f64(lib, a) == NO_DEVICE
    assert _plan(5)[1]["ntiles"] == 1
