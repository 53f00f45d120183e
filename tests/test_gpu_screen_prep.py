"""The setup kernels of the two safe screens against float64, through the hooks admm_hip_test_wide_screen_prep and
admm_hip_test_sbp_screen_prep: wide_screen_prep_kernel (fp16 copy), wide_screen_prep8_kernel (8-bit code), wide_screen_rate8_kernel
(which picks the format) of lasso_wide.hip, and sbp_screen_prep_kernel of sharing_bp.hip.  The solvers' own tests see these kernels
only through "the screened run is bit-identical to the unscreened one", which holds on Gaussian data with a bound half the size.

What is asserted is derived, never measured:
  copy     fp16: the bits of X.astype(float16) (sbp: of A.astype(float32).astype(float16), the kernel rounds twice), a rounding that is
           not finite stored as +0; 8-bit: codes in [-127, 127], scale_j = float32(max|x|) / float32(127) to the bit, every entry within
           half a step (1 + 1e-6) of its code; rows [n, ldh) zero although the device rows [n, ldx) hold NaN and the copy was 0xff.
  bound    B_j = the kernel's formula in float64 ON THE RETURNED COPY (the copy the screen will read):
               wide  ||x - c|| + 2 gamma_n max(||x||, ||c||),  gamma_n = 1.001 n 2^-24
               sbp   ||a - c|| + 1.01 (n + 4) 2^-24 max(||a||, ||c||)
           safety s_j >= B_j with no tolerance (the kernel's own factor 1 + 1e-6 and its round-up dwarf the summation error of float64
           at n <= 8192); tightness s_j <= B_j (1 + 1.2e-6) + 2^-149: the factor 1e-6 and one float round-up, which is 2^-23 relative
           or, for a subnormal result, one step of 2^-149.  A zero column: exactly 0.  A NaN / Inf column, or a bound beyond FLT_MAX: +Inf.
  placement  column j at [(j % NW) * S + j // NW] of the [NW * S] arrays, every other slot exactly 0, S a multiple of 64.
  rate     each partial = the sum of min(r_j, 4) over its four columns, r_j by the kernel's formula (4 gamma_n, not 2), 1e-6 relative.
Figures are printed ("screen_prep ..." lines, pytest -s): profiles/screen_tests.md."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS = [1, 7, 8, 9, 15, 16, 17, 255, 257, 1031, 4100, 8192]
PS = [1, 3, 4, 5, 67]
NWS = [1, 4, 96]
NAN_FILL = 0x7FC00000
FLT_MAX = float(np.finfo(np.float32).max)
U24 = 2.0 ** -24


# ---- columns
def _put(col, values, start=0):
    """values at consecutive rows (modulo the length: a short column keeps the last ones)"""
    for k, v in enumerate(values):
        col[(start + k) % len(col)] = v
    return col


def _special_columns(n, rng, wide):
    """(name, column) pairs, float64; the wide tests narrow them to float32."""
    g = lambda: rng.standard_normal(n)                                   # noqa: E731
    sign = lambda: np.where(rng.random(n) < 0.5, -1.0, 1.0)              # noqa: E731
    cols = [
        ("zero", np.zeros(n)),
        ("negzero", np.full(n, -0.0)),
        ("single", _put(np.zeros(n), [1.7], n // 2)),
        ("negzero_mixed", _put(g(), [-0.0, -0.0, 0.0], 1)),
        ("f16max", _put(g(), [65504.0, 65519.9, 65520.0, -65520.0, -65504.0])),            # 65519.9 -> 65504; +-65520 -> Inf -> stored 0
        ("f16_subnormal", g() * 2.0 ** -19),                                                # fp16 subnormals: below 2^-14, steps of 2^-24
        ("below_half_subnormal", rng.uniform(-1, 1, n) * 2.0 ** -26),                       # |x| < 2^-25: rounds to +-0
        ("ties", sign() * np.where(np.arange(n) % 2 == 0, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11)),      # -> 1 and 1 + 2^-9 (even mantissas)
        ("near_flt_max", _put(g(), [3.0e38], n // 3)),
        ("flt_max", _put(g(), [-FLT_MAX], n // 3)),                                          # its bound exceeds FLT_MAX: +Inf
        ("nan", _put(g(), [np.nan], n // 2)),
        ("inf", _put(g(), [np.inf], n // 4)),
        ("neg_inf", _put(g(), [-np.inf], n - 1)),
        ("max_is_negative", _put(np.clip(g(), -3, 3), [-5.0], n // 2)),
        ("constant", np.full(n, 0.37)),
        ("max_is_subnormal_float", _put(rng.integers(-100, 101, n) * 2.0 ** -149, [-100 * 2.0 ** -149], n // 2)),      # scale: 100 / 127 steps -> 2^-149
    ]
    if not wide:      # double only: rounds to 1 + 2^-10 directly, to 1 through float (1 + 2^-11 is then an exact tie)
        cols.append(("double_rounding", sign() * (1 + 2.0 ** -11 + 2.0 ** -30)))
    return cols


_POOL = {}


def _matrix(n, p, wide):
    """p columns: the special ones where they fit (all of them at p = 67, a window of them at small p), Gaussian otherwise."""
    key = (n, p, wide)
    if key not in _POOL:
        rng = np.random.default_rng(1000 * n + p)
        special = _special_columns(n, rng, wide)
        if p >= len(special) + 1:
            picked = special
        else:
            off = {1: 0, 3: 0, 4: 2, 5: 5}.get(p, 0)
            rot = special[off:] + special[:off]
            picked = rot[:p - 1]                                       # one Gaussian column stays
        names = ["gauss"] * p
        M = rng.standard_normal((n, p)) * rng.choice([1.0, 37.0, 1e-3], p)
        # spread the special columns over the slots (not only the first ones): column j = 1 + 3 k modulo p where that is free
        slots = list(range(p))
        for k, (name, col) in enumerate(picked):
            j = slots.pop((1 + 3 * k) % len(slots)) if len(slots) > 1 else slots.pop()
            M[:, j] = col
            names[j] = name
        M = np.asfortranarray(M.astype(np.float32) if wide else M)
        M.setflags(write=False)
        _POOL[key] = (M, names)
    return _POOL[key]


# ---- the hooks
def _wide_prep(X, fmt, nw, pad_fill=NAN_FILL):
    from admm_amd import _lib
    n, p = X.shape
    assert X.dtype == np.float32 and X.flags.f_contiguous
    epl = 16 if fmt == 8 else 8
    ldh = (n + epl - 1) // epl * epl
    S = ((p + nw - 1) // nw + 63) // 64 * 64
    copy = np.full(p * ldh, 0x55, np.int8 if fmt == 8 else np.uint16)
    s, scale = np.full(nw * S, np.nan, np.float32), np.full(nw * S, np.nan, np.float32)
    rate, info = np.full((p + 3) // 4, np.nan), np.zeros(4, np.int64)
    fp, dp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)
    _lib.check(_lib.load().admm_hip_test_wide_screen_prep(X.ctypes.data_as(fp), n, p, fmt, nw, pad_fill, copy.ctypes.data_as(ctypes.c_void_p), copy.size,
                                                          s.ctypes.data_as(fp), scale.ctypes.data_as(fp) if fmt == 8 else None, rate.ctypes.data_as(dp),
                                                          info.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))))
    assert list(info) == [ldh, S, nw, (n + 15) // 16 * 16] and S % 64 == 0
    return dict(copy=copy.reshape(p, ldh).T, s=s, scale=scale if fmt == 8 else None, rate=rate, S=S, ldh=ldh)


def _sbp_prep(A, lda_extra, pad_fill=NAN_FILL):
    from admm_amd import _lib
    n, p = A.shape
    assert A.dtype == np.float64 and A.flags.f_contiguous
    ldh = (n + 7) // 8 * 8
    copy, s, info = np.full(p * ldh, 0x5555, np.uint16), np.full(p, np.nan, np.float32), np.zeros(2, np.int64)
    _lib.check(_lib.load().admm_hip_test_sbp_screen_prep(A.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), n, p, lda_extra, pad_fill,
                                                         copy.ctypes.data_as(ctypes.c_void_p), copy.size, s.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                         info.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))))
    assert list(info) == [ldh, (n + 31) // 32 * 32 + lda_extra]
    return dict(copy=copy.reshape(p, ldh).T, s=s, ldh=ldh)


# ---- the references
def _fp16_bits(Xf32):
    """X rounded to fp16 (round to nearest even, as numpy rounds), a rounding that is not finite stored as +0"""
    with np.errstate(all="ignore"):
        h = Xf32.astype(np.float16)
    h[~np.isfinite(h)] = 0.0
    return h.view(np.uint16)


def _assert_bounds(s, X64, back64, gamma_term, bad, names, what):
    """s [p] against B_j = ||x - c|| + gamma_term * max(||x||, ||c||) in float64 on the returned copy; returns the largest s / B - 1."""
    worst = 0.0
    with np.errstate(all="ignore"):
        e = np.sqrt(((X64 - back64) ** 2).sum(axis=0))
        big = np.sqrt(np.maximum((X64 ** 2).sum(axis=0), (back64 ** 2).sum(axis=0)))
        B = e + gamma_term * big
    for j in range(X64.shape[1]):
        tag = (what, j, names[j], float(s[j]), float(B[j]))
        if bad[j] or not B[j] * (1 + 1e-6) <= FLT_MAX:
            assert s[j] == np.inf, tag
            continue
        assert np.isfinite(s[j]) and float(s[j]) >= B[j], ("unsafe bound",) + tag
        assert float(s[j]) <= B[j] * (1 + 1.2e-6) + 2.0 ** -149, ("loose bound",) + tag
        if not X64[:, j].any():
            assert s[j] == 0 and not np.signbit(s[j]), tag
        if B[j] > 2.0 ** -120:
            worst = max(worst, float(s[j]) / B[j] - 1)
    return worst


def _placed(arr, p, nw, S, what):
    """the [NW * S] array's entries of columns 0 .. p - 1; every other slot must be exactly +0"""
    j = np.arange(p)
    pos = (j % nw) * S + j // nw
    assert len(set(pos.tolist())) == p
    rest = np.ones(nw * S, bool)
    rest[pos] = False
    assert not arr.view(np.uint32)[rest].any(), (what, "a slot that belongs to no column was written", np.nonzero(arr.view(np.uint32) * rest)[0][:5])
    return arr[pos]


def _rate_reference(X, n):
    """wide_screen_rate8_kernel's r_j: the code's step in float (as the kernel), the sums in float64"""
    with np.errstate(all="ignore"):
        mx = np.fmax.reduce(np.abs(X), axis=0, initial=np.float32(0)).astype(np.float32)      # fmaxf: a NaN is skipped
        sc = mx / np.float32(127)
        q = np.clip(np.rint(X / sc), -127, 127).astype(np.float64)
        db = np.where(sc > 0, sc.astype(np.float64) * q, 0.0)
        x64 = X.astype(np.float64)
        e2, x2 = ((x64 - db) ** 2).sum(axis=0), (x64 ** 2).sum(axis=0)
        gn = 1.001 * n * U24
        r = np.where(x2 > 0, (np.sqrt(e2) + 4.0 * gn * np.sqrt(x2)) * np.sqrt(float(n)) / np.sqrt(x2), 0.0)
        r[~(r <= 4.0)] = 4.0
    return r


def _same(a, b):
    return all((a[k] is None and b[k] is None) or np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("copy", "s", "scale", "rate"))


@pytest.mark.parametrize("fmt", [16, 8])
@pytest.mark.parametrize("n", NS)
def test_wide_screen_setup_against_float64(n, fmt):
    worst_tight, worst_code, worst_rate, ncalls = 0.0, 0.0, 0.0, 0
    for p in PS:
        X, names = _matrix(n, p, True)
        X64 = X.astype(np.float64)
        with np.errstate(all="ignore"):
            finite = np.isfinite(X).all(axis=0)
            # the 8-bit kernel counts an entry beyond 3e38 as not finite (its comment): scale 0, bound +Inf
            bad = ~finite if fmt == 16 else ~(np.abs(X) <= np.float32(3.0e38)).all(axis=0)
        rate_ref = _rate_reference(X, n)
        for nw in NWS:
            what = f"wide fmt {fmt} n {n} p {p} nw {nw}"
            out = _wide_prep(X, fmt, nw)
            ncalls += 1
            copy, S = out["copy"], out["S"]
            assert not copy[n:].any(), (what, "rows [n, ldh) of the copy must be zero")
            s = _placed(out["s"], p, nw, S, what + " s")
            if fmt == 16:
                want = _fp16_bits(X)
                assert np.array_equal(copy[:n], want), (what, "fp16 bits", [names[j] for j in np.nonzero((copy[:n] != want).any(axis=0))[0]])
                back = copy[:n].view(np.float16).astype(np.float64)
            else:
                scale = _placed(out["scale"], p, nw, S, what + " scale")
                q = copy[:n].astype(np.int64)
                assert q.min() >= -127 and q.max() <= 127, what
                with np.errstate(all="ignore"):
                    mx = np.abs(X).max(axis=0).astype(np.float32)
                    want_scale = np.where(bad, np.float32(0), mx / np.float32(127)).astype(np.float32)
                assert np.array_equal(scale.view(np.uint32), want_scale.view(np.uint32)), (what, "scale", names, scale, want_scale)
                assert not q[:, bad].any(), (what, "a column that is not finite has all codes 0")
                back = scale.astype(np.float64) * q
                ok = ~bad
                err = np.abs(back[:, ok] - X64[:, ok])
                half = scale[ok].astype(np.float64) / 2
                assert (err <= half * (1 + 1e-6)).all(), (what, "an entry further than half a step from its code", float((err / np.where(half > 0, half, 1)).max()))
                if (half > 0).any():
                    worst_code = max(worst_code, float((err[:, half > 0] / half[half > 0]).max()))
            worst_tight = max(worst_tight, _assert_bounds(s, X64, back, 2.0 * 1.001 * n * U24, bad, names, what))
            # the format choice: partial b = the sum of min(r_j, 4) over columns 4 b .. 4 b + 3 below p
            rp = np.concatenate([rate_ref, np.zeros(-p % 4)]).reshape(-1, 4)
            want_rate = (rp[:, 0] + rp[:, 1]) + (rp[:, 2] + rp[:, 3])
            assert out["rate"].shape == want_rate.shape and np.all(np.abs(out["rate"] - want_rate) <= 1e-6 * want_rate), (what, out["rate"], want_rate)
            if want_rate.max() > 0:
                worst_rate = max(worst_rate, float(np.max(np.abs(out["rate"] - want_rate)[want_rate > 0] / want_rate[want_rate > 0])))
            for j in np.nonzero(~X64.any(axis=0))[0]:
                assert rate_ref[j] == 0, (what, "a zero column contributes nothing to the rate")
            if nw == 4:
                assert _same(out, _wide_prep(X, fmt, nw)), (what, "a second call returned other bytes")
                assert _same(out, _wide_prep(X, fmt, nw, pad_fill=0x3F800000)), (what, "the rows [n, ldx) of the device matrix were read")
                ncalls += 2
    print(f"screen_prep wide fmt {fmt} n {n}: {ncalls} calls, s / B - 1 at most {worst_tight:.3e}, code error at most {worst_code:.7f} of half a step, "
          f"rate partials within {worst_rate:.1e}")


@pytest.mark.parametrize("lda_extra", [0, 8])
@pytest.mark.parametrize("n", NS)
def test_sbp_screen_setup_against_float64(n, lda_extra):
    worst_tight = 0.0
    for p in PS:
        A, names = _matrix(n, p, False)
        what = f"sbp n {n} p {p} lda_extra {lda_extra}"
        out = _sbp_prep(A, lda_extra)
        copy = out["copy"]
        assert not copy[n:].any(), (what, "rows [n, ldh) of the copy must be zero")
        with np.errstate(all="ignore"):
            want = _fp16_bits(A.astype(np.float32))
            bad = ~np.isfinite(A).all(axis=0)
        assert np.array_equal(copy[:n], want), (what, "fp16 bits", [names[j] for j in np.nonzero((copy[:n] != want).any(axis=0))[0]])
        back = copy[:n].view(np.float16).astype(np.float64)
        worst_tight = max(worst_tight, _assert_bounds(out["s"], A, back, 1.01 * (n + 4.0) * U24, bad, names, what))
        again, other_fill = _sbp_prep(A, lda_extra), _sbp_prep(A, lda_extra, pad_fill=0x3FF00000)
        for o, why in ((again, "a second call returned other bytes"), (other_fill, "rows beyond n of the device matrix were read")):
            assert o["copy"].tobytes() == copy.tobytes() and o["s"].tobytes() == out["s"].tobytes(), (what, why)
    print(f"screen_prep sbp n {n} lda_extra {lda_extra}: s / B - 1 at most {worst_tight:.3e}")


def test_the_special_columns_are_what_they_claim():
    """the inputs themselves (no kernel): what the fp16 rounding of the special columns must be, so that the bit comparison above
    compares with the intended cases"""
    X, names = _matrix(257, 67, True)
    col = lambda name: X[:, names.index(name)]              # noqa: E731
    h = lambda name: _fp16_bits(col(name)).view(np.float16).astype(np.float64)      # noqa: E731
    assert set(np.abs(h("ties")).tolist()) == {1.0, 1 + 2.0 ** -9}
    f = col("f16max")
    assert f[1] == np.float32(65519.9) and list(h("f16max")[:5]) == [65504.0, 65504.0, 0.0, 0.0, -65504.0]
    assert not h("below_half_subnormal").any() and np.abs(col("below_half_subnormal")).max() < 2.0 ** -25 and col("below_half_subnormal").any()
    sub = np.abs(h("f16_subnormal"))
    assert ((sub > 0) & (sub < 2.0 ** -14)).sum() > 200
    assert 0 < np.abs(col("max_is_subnormal_float")).max() < np.finfo(np.float32).tiny
    assert np.abs(col("max_is_negative")).argmax() == 257 // 2 and col("max_is_negative")[257 // 2] < 0
    A, an = _matrix(257, 67, False)
    d = A[:, an.index("double_rounding")]
    assert not np.array_equal(d.astype(np.float16), d.astype(np.float32).astype(np.float16))
    assert sorted(set(names)) == sorted(set(n_ for n_, _ in _special_columns(4, np.random.default_rng(0), True)) | {"gauss"})
