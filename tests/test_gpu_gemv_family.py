"""Every launch form of the shared streaming mat-vec (gemv_kernels.h: gemv_t_body through launch_gemv_t with one and two right-hand
sides, GemvT::run, the chain GemvT::run_partials -> GemvT::run_from on both of its routes, gemv_t_batch_kernel, plain and non-temporal
loads, the big64 plan) through the hook admm_hip_test_gemv_t_ex, PARTIAL ROW BY PARTIAL ROW against float64 / int64, and the wide
solver's Gram-free operator w = X (X'v) (prep.hip: gemv_n_partial_kernel) through admm_hip_test_wide_op.

The hook stores a matrix as the callers do (leading dimension round_up(m, 32) + 32 here, rows [m, round_up(m, 32)) zero) and makes
everything the kernel has no business with hostile: the rows beyond are NaN, the tails of the right-hand vectors are NaN, every partial
and output buffer starts as a NaN bit pattern that has to survive wherever the launch does not write.  Shapes are chosen by the plan they
produce (_plan restates plan_gemv_t's segmentation), and every test asserts that plan, the route and the loads taken from info_out.

Tolerances: those of tests/test_gpu_kernels.py::test_gemv_t_vs_numpy, per partial row: 2e-6 (float) / 1e-14 (double) of
max(|A|'|v|) over the row's own segment.  A chain A2'(A1'v) is held to the same factor of max(|A2|'(|A1|'|v|)), the scale at which both
products' roundings arrive in the result; the Gram-free operator to twice that factor (two chained products).
Every test prints the worst figure it met ("gemv_family ..." lines, pytest -s): profiles/gemv_family_tests.md."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FILL = 0x7FF8BEEF7FC0BEEF                      # a NaN pattern in both widths (float: the low 32 bits)
TOL = {np.float32: 2e-6, np.float64: 1e-14}
ONE_PASS = {np.float32: 256, np.float64: 128}  # rows of one wave pass: the smallest segment a plan can have
EXACT = {np.float32: 2 ** 24, np.float64: 2 ** 53}
DTYPES = [np.float32, np.float64]
EXTRA = 32                                     # NaN rows behind every column
CHAIN_ROWS = 12                                # GemvT::kChainRows
ROUTE_PLAIN, ROUTE_KERNEL, ROUTE_REDUCE = 0, 1, 2


def _ru(a, b):
    return -(-a // b) * b


def _plan(m, dtype, nrhs=1, cap=0):
    """plan_gemv_t's row segmentation: (nseg, seg_len)."""
    size = np.dtype(dtype).itemsize
    wave_pass = 64 * (16 // size)
    max_rows = (160 * 1024 // 4 - 512) // (nrhs * size) // wave_pass * wave_pass
    if cap > 0:
        max_rows = min(max_rows, max(wave_pass, cap // wave_pass * wave_pass))
    nseg = -(-m // max_rows)
    seg_len = _ru(-(-m // nseg), 32)
    return -(-m // seg_len), seg_len


def _m_for(nseg, dtype):
    """Rows that one-pass segments split into `nseg` partial rows; from 8 (float) / 7 (double) rows on the last segment has 13 rows."""
    return ONE_PASS[dtype] * (nseg - 1) + 13


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _is_fill(a):
    return bool((_bits(a) == (FILL & 0xFFFFFFFF if a.dtype == np.float32 else FILL)).all())


def _same(a, b):
    return a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


class _Product:
    def __init__(self, info, part, y, k):
        self.nseg, self.seg_len, self.gpw, self.grid, self.nt, self.route, self.vparts, self.width = (int(x) for x in info)
        self.k, self.stride = k, _ru(k, 32)
        self.raw, self.y_raw = part, y
        self.rows = part[:, :self.nseg * self.stride].reshape(part.shape[0], self.nseg, self.stride)      # [nrhs][nseg][stride]
        self.y = None if y is None else y[:k]

    def untouched_is_fill(self):
        """Entries beyond k of every partial row, everything behind the nseg rows and the tail of y keep the pattern."""
        ok = _is_fill(self.rows[:, :, self.k:]) and _is_fill(self.raw[:, self.nseg * self.stride:])
        return ok and (self.y_raw is None or _is_fill(self.y_raw[self.k:]))

    def grid_is_consistent(self):
        ngroups = -(-self.k // 4)
        return self.gpw >= 4 and self.gpw % 4 == 0 and self.grid == self.nseg * -(-ngroups // self.gpw)


def _run(dtype, form, prods, nrhs=1, nt=-1, cap=0, frm=None, skip=None, rows=None):
    """prods: [(A [m, k] Fortran, v [nrhs, m] or None)].  One call of the hook; a _Product per product."""
    from admm_amd import _lib
    n = len(prods)
    ms, ks = [a.shape[0] for a, _ in prods], [a.shape[1] for a, _ in prods]
    for a, v in prods:
        assert a.dtype == dtype and a.flags.f_contiguous and (v is None or (v.dtype == dtype and v.shape == (nrhs, a.shape[0]) and v.flags.c_contiguous))
    capacity = max(((rows or _plan(m, dtype, nrhs, cap)[0]) + 2) * _ru(k, 32) for m, k in zip(ms, ks))      # two guard rows behind the last
    parts = [np.zeros((nrhs, capacity), dtype) for _ in prods]
    ys = [np.zeros(_ru(k, 32), dtype) for k in ks]
    info = (ctypes.c_longlong * (8 * n))()
    ptrs = lambda xs: (ctypes.c_void_p * n)(*[None if x is None else x.ctypes.data for x in xs])      # noqa: E731
    ints = lambda xs: None if xs is None else (ctypes.c_int * n)(*xs)                                   # noqa: E731
    has_y = form in (1, 2)
    _lib.check(_lib.load().admm_hip_test_gemv_t_ex(int(dtype == np.float64), form, nrhs, nt, cap, EXTRA, FILL, n, ints(ms), ints(ks),
                                                   ptrs([a for a, _ in prods]), ptrs([v for _, v in prods]), ints(frm), ints(skip), ptrs(parts), capacity,
                                                   ptrs(ys) if has_y else None, info))
    return [_Product(info[8 * i:8 * i + 8], parts[i], ys[i] if has_y and i == n - 1 else None, ks[i]) for i in range(n)]


def _row_refs(A, v, seg_len):
    """Per segment: (float64 A[seg]'v[seg], max(|A[seg]|'|v[seg]|))."""
    A64, v64 = A.astype(np.float64), v.astype(np.float64)
    out = []
    for r0 in range(0, A.shape[0], seg_len):
        a, x = A64[r0:r0 + seg_len], v64[r0:r0 + seg_len]
        out.append((a.T @ x, float((np.abs(a).T @ np.abs(x)).max())))
    return out


def _worst_row_error(p, A, V):
    """Largest error of any partial row of any right-hand side, in units of its segment's scale."""
    worst = 0.0
    for r in range(V.shape[0]):
        refs = _row_refs(A, V[r], p.seg_len)
        assert len(refs) == p.nseg
        for s, (ref, scale) in enumerate(refs):
            worst = max(worst, float(np.abs(p.rows[r, s, :p.k] - ref).max()) / max(scale, np.finfo(np.float64).tiny))
    return worst


def _sum_rows(rows):
    """The partial rows summed in row order in their own type (the staging loop, reduce_partials_kernel)."""
    acc = np.zeros(rows.shape[1], rows.dtype)
    for r in rows:
        acc = acc + r
    return acc


def _gauss(seed, m, k, dtype, nrhs=1):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(rng.standard_normal((m, k)).astype(dtype)), np.ascontiguousarray(rng.standard_normal((nrhs, m)).astype(dtype))


def _ints(seed, m, k, dtype, lim, nrhs=1):
    """Small integers as tests/test_gpu_symv_packed.py::_ints draws them: (A, V in `dtype`, A and V as int64)."""
    rng = np.random.default_rng(seed)
    Ai = rng.integers(-lim, lim + 1, size=(m, k)).astype(np.int64)
    Vi = rng.integers(-lim, lim + 1, size=(nrhs, m)).astype(np.int64)
    return np.asfortranarray(Ai.astype(dtype)), np.ascontiguousarray(Vi.astype(dtype)), Ai, Vi


def _report(what, dtype, **figures):
    print("gemv_family %s %s: %s" % (what, np.dtype(dtype).name, ", ".join("%s=%s" % (k, ("%.3g" % v) if isinstance(v, float) else v) for k, v in figures.items())))


# ---------------------------------------------------------------- per partial row against float64: edges and segments

EDGE_M, EDGE_K = (1, 31, 32, 33, 255, 256, 257, 1027), (1, 3, 4, 5, 15, 17, 130)


@pytest.mark.parametrize("nrhs", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_edges_per_partial_row(dtype, nrhs):
    """m around the 32-row padding, one wave pass and the 4 x 256 staging step, k with a clamped duplicate column (k % 4) and fewer
    than 16 columns (groups_per_wg rounds up to the 4 waves), under the default plan and under one-pass segments; launch_gemv_t with
    one and two right-hand sides, and GemvT::run on the same inputs (its y is the ordered sum of those rows, bit for bit)."""
    worst, plans = 0.0, set()
    for cap in (0, ONE_PASS[dtype]):
        for m in EDGE_M:
            for k in EDGE_K:
                A, V = _gauss(1000 * m + k, m, k, dtype, nrhs)
                p, = _run(dtype, 0, [(A, V)], nrhs=nrhs, cap=cap)
                assert (p.nseg, p.seg_len) == _plan(m, dtype, nrhs, cap) and p.grid_is_consistent() and p.width == p.grid, (m, k, cap)
                assert (p.nt, p.route, p.vparts) == (0, ROUTE_PLAIN, 1)
                assert p.untouched_is_fill(), (m, k, cap)
                err = _worst_row_error(p, A, V)
                assert err < TOL[dtype], (m, k, cap, err)
                worst = max(worst, err)
                plans.add(p.nseg)
                if nrhs == 1:
                    q, = _run(dtype, 1, [(A, V)], cap=cap)
                    assert (q.nseg, q.seg_len, q.grid) == (p.nseg, p.seg_len, p.grid) and q.untouched_is_fill()
                    assert _same(q.y, _sum_rows(p.rows[0])[:k]), (m, k, cap)
                    if q.nseg > 1:
                        assert _same(q.rows, p.rows)
                    else:
                        assert _is_fill(q.raw)                    # the one-segment shortcut writes y alone
    assert plans == ({1, 2, 3, 9} if dtype == np.float64 else {1, 2, 5})
    _report("form 0 edges nrhs=%d" % nrhs, dtype, worst=worst, nseg=sorted(plans))


SEGMENTS = (2, 7, 8, 9, 12, 13, 25)


@pytest.mark.parametrize("dtype", DTYPES)
def test_segments_per_partial_row(dtype):
    """One-pass segments at small m: 2 .. 25 partial rows, from 8 rows on with a last segment of 13 rows (shorter than the 32-row
    alignment, than a vector load's worth of lanes and than everything the kernel rounds to)."""
    worst, k = 0.0, 37
    for nseg in SEGMENTS:
        m = _m_for(nseg, dtype)
        A, V = _gauss(7 * m, m, k, dtype, 2)
        p, = _run(dtype, 0, [(A, V)], nrhs=2, cap=ONE_PASS[dtype])
        assert p.nseg == nseg and (p.nseg, p.seg_len) == _plan(m, dtype, 2, ONE_PASS[dtype]) and p.grid_is_consistent()
        if nseg >= 8:
            assert m - (nseg - 1) * p.seg_len == 13
        assert p.untouched_is_fill()
        err = _worst_row_error(p, A, V)
        assert err < TOL[dtype], (nseg, err)
        q, = _run(dtype, 1, [(A, V[:1])], cap=ONE_PASS[dtype])
        assert q.nseg == nseg and _same(q.rows[0], p.rows[0]) and _same(q.y, _sum_rows(q.rows[0])[:k]) and q.untouched_is_fill()
        ref = A.astype(np.float64).T @ V[0].astype(np.float64)
        scale = (np.abs(A.astype(np.float64)).T @ np.abs(V[0].astype(np.float64))).max()
        assert np.abs(q.y - ref).max() / scale < TOL[dtype]
        worst = max(worst, err)
    _report("forms 0 and 1, one-pass segments", dtype, worst=worst, nseg=list(SEGMENTS))


# ---------------------------------------------------------------- chains


def _chain_case(dtype, m1, k1, k2, cap, seed):
    A1, V = _gauss(seed, m1, k1, dtype)
    A2, _ = _gauss(seed + 1, k1, k2, dtype)
    return A1, V, A2


def _check_chain(dtype, A1, V, A2, cap, route):
    """Form 2 on (A1, A2): the first product's rows as form 0 leaves them; the second product bit-identical to form 0 on the first's
    rows summed in row order on the host, and within tolerance of float64 A2'(A1'v).  Returns (first, second, error)."""
    a, b = _run(dtype, 2, [(A1, V), (A2, None)], cap=cap)
    f, = _run(dtype, 0, [(A1, V)], cap=cap)
    assert _same(a.rows, f.rows) and a.untouched_is_fill() and b.untouched_is_fill()
    assert (b.vparts, b.route) == (a.nseg, route), (b.vparts, b.route)
    assert (a.nt, b.nt) == (0, 0) and a.grid_is_consistent() and b.grid_is_consistent() and (a.width, b.width) == (a.grid, b.grid)
    u = _sum_rows(a.rows[0])[:a.k]
    g, = _run(dtype, 0, [(A2, u[None, :].copy())], cap=cap)
    assert (g.nseg, g.seg_len, g.grid) == (b.nseg, b.seg_len, b.grid)
    if b.nseg > 1:
        assert _same(b.rows, g.rows)
        assert _same(b.y, _sum_rows(b.rows[0])[:b.k])
    else:
        assert _is_fill(b.raw) and _same(b.y, g.rows[0, 0, :g.k])
    A1d, A2d, vd = A1.astype(np.float64), A2.astype(np.float64), V[0].astype(np.float64)
    ref, scale = A2d.T @ (A1d.T @ vd), (np.abs(A2d).T @ (np.abs(A1d).T @ np.abs(vd))).max()
    err = float(np.abs(b.y - ref).max() / scale)
    assert err < TOL[dtype], err
    # and per partial row of the second product, against float64 on the float64 right-hand side
    u64, uabs = A1d.T @ vd, np.abs(A1d).T @ np.abs(vd)
    rows = g.rows[0] if b.nseg == 1 else b.rows[0]
    for s in range(b.nseg):
        seg = slice(s * b.seg_len, (s + 1) * b.seg_len)
        row_scale = (np.abs(A2d[seg]).T @ uabs[seg]).max()
        assert np.abs(rows[s, :b.k] - A2d[seg].T @ u64[seg]).max() / row_scale < TOL[dtype], s
    return a, b, err


@pytest.mark.parametrize("vparts", [1, 2, 3, 7, 8, 9, 12, 13, 25])
@pytest.mark.parametrize("dtype", DTYPES)
def test_chain_sums_the_partial_rows_in_order(dtype, vparts):
    """The right-hand side arrives in `vparts` partial rows: one (a plain vector), up to 12 summed eight at a time while the segment is
    staged (the 8 / 9 boundary of that loop, the last round of 1, 4 and 5 rows), 13 and 25 summed by a reduce launch into a single
    row.  The second product has 2 (float) / 3 (double) segments of its own, so that the struct's routes are the ones that run."""
    cap = ONE_PASS[dtype]
    A1, V, A2 = _chain_case(dtype, _m_for(vparts, dtype), 300, 37, cap, 100 + vparts)
    route = ROUTE_PLAIN if vparts == 1 else ROUTE_KERNEL if vparts <= CHAIN_ROWS else ROUTE_REDUCE
    a, b, err = _check_chain(dtype, A1, V, A2, cap, route)
    assert a.nseg == vparts and b.nseg == _plan(300, dtype, 1, cap)[0] > 1
    _report("form 2 chain vparts=%d route=%d" % (vparts, route), dtype, worst=err, nseg2=b.nseg, seg_len2=b.seg_len, grid2=b.grid)


@pytest.mark.parametrize("dtype", DTYPES)
def test_chain_last_segment_shorter_than_a_staging_step(dtype):
    """Segments of up to 1280 rows: the second product (1500 rows) has two of 768 and 732, both shorter than the 4 x 256 rows a
    staging step covers and the last no multiple of 256 -- the clamp min(i0 + e * 256, len - 1) -- under 3 partial rows; and the
    one-segment shortcut of run_from (45 rows), which stages 25 rows in the kernel whatever their number."""
    A1, V, A2 = _chain_case(dtype, 3000, 1500, 41, 1280, 5)
    a, b, err = _check_chain(dtype, A1, V, A2, 1280, ROUTE_KERNEL)
    assert (a.nseg, a.seg_len, b.nseg, b.seg_len) == (3, 1024, 2, 768)
    _report("form 2 chain, 732-row last segment", dtype, worst=err, vparts=b.vparts)
    cap = ONE_PASS[dtype]
    A1, V, A2 = _chain_case(dtype, _m_for(25, dtype), 45, 19, cap, 6)
    a, b, err = _check_chain(dtype, A1, V, A2, cap, ROUTE_KERNEL)
    assert (a.nseg, b.nseg) == (25, 1)
    _report("form 2 chain, one-segment shortcut over 25 rows", dtype, worst=err)


# ---------------------------------------------------------------- exact data


@pytest.mark.parametrize("dtype", DTYPES)
def test_small_integers_are_exact_in_every_form(dtype):
    """Every partial sum below 2^24 (float) / 2^53 (double), asserted on the int64 reference: every partial row and every reduced
    vector equals the int64 product, whatever the order of the sums, in forms 0 (two right-hand sides), 1, 2 (both routes) and 3."""
    cap = ONE_PASS[dtype]
    for nseg in (1, 9, 13):
        m = _m_for(nseg, dtype)
        A, V, Ai, Vi = _ints(m, m, 300, dtype, 2, nrhs=2)
        B, _, Bi, _ = _ints(m + 1, 300, 290, dtype, 1)
        C, _, Ci, _ = _ints(m + 2, 290, 29, dtype, 1)
        u = Ai.T @ Vi[0]
        w = Bi.T @ u
        # (a partial sum of a product is bounded by the sum of its terms' magnitudes, in any order: |M|'|x| for the x the product really gets)
        assert max((np.abs(Ai).T @ np.abs(Vi).T).max(), (np.abs(Bi).T @ np.abs(u)).max(), (np.abs(Ci).T @ np.abs(w)).max()) < EXACT[dtype]
        p, = _run(dtype, 0, [(A, V)], nrhs=2, cap=cap)
        q, = _run(dtype, 1, [(A, V[:1])], cap=cap)
        assert p.nseg == q.nseg == nseg and p.untouched_is_fill() and q.untouched_is_fill()
        for s in range(nseg):
            seg = slice(s * p.seg_len, (s + 1) * p.seg_len)
            for r in range(2):
                assert np.array_equal(p.rows[r, s, :p.k].astype(np.int64), Ai[seg].T @ Vi[r, seg]), (nseg, s, r)
        assert np.array_equal(q.y.astype(np.int64), u)
        # the chain A -> B on the route the struct takes for `nseg` rows, then B -> C, in form 2 and in the batched launch's second stage
        a, b = _run(dtype, 2, [(A, V[:1]), (B, None)], cap=cap)
        route = ROUTE_PLAIN if nseg == 1 else ROUTE_KERNEL if nseg <= CHAIN_ROWS else ROUTE_REDUCE
        assert b.nseg > 1 and (a.nseg, b.vparts, b.route) == (nseg, nseg, route)
        assert np.array_equal(b.y.astype(np.int64), w)
        for s in range(b.nseg):
            seg = slice(s * b.seg_len, (s + 1) * b.seg_len)
            assert np.array_equal(b.rows[0, s, :b.k].astype(np.int64), Bi[seg].T @ u[seg]), (nseg, s)
        uT = u.astype(dtype)[None, :].copy()
        c, d = _run(dtype, 2, [(B, uT), (C, None)], cap=cap)
        assert d.nseg > 1 and (d.vparts, d.route) == (c.nseg, ROUTE_KERNEL) and np.array_equal(d.y.astype(np.int64), Ci.T @ w)
        x, y, z = _run(dtype, 3, [(A, V[:1]), (B, uT), (C, None)], cap=cap, frm=[-1, -1, 1])
        assert (z.vparts, z.route) == (y.nseg, ROUTE_KERNEL) and _same(z.rows, d.rows) and _same(y.rows, c.rows) and _same(x.rows, a.rows)
        for s in range(z.nseg):
            seg = slice(s * z.seg_len, (s + 1) * z.seg_len)
            assert np.array_equal(z.rows[0, s, :z.k].astype(np.int64), Ci[seg].T @ w[seg])
    _report("exact integers, forms 0-3", dtype, worst=0.0)


# ---------------------------------------------------------------- non-temporal against plain loads


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_temporal_loads_give_the_same_bits(dtype):
    """nt = 0 and nt = 1 forced on the same inputs: every partial row and every reduced vector bit-identical, in forms 0 (both
    instantiations), 2 (both routes) and 3; info_out says which loads ran."""
    cap = ONE_PASS[dtype]
    m = _m_for(9, dtype)
    A, V = _gauss(21, m, 131, dtype, 2)
    B, W = _gauss(22, 700, 37, dtype)
    C, _ = _gauss(23, 131, 45, dtype)
    A13, V13 = _gauss(24, _m_for(13, dtype), 300, dtype)
    C13, _ = _gauss(25, 300, 21, dtype)
    calls = [dict(form=0, prods=[(A, V)], nrhs=2), dict(form=0, prods=[(A, V[:1])]), dict(form=2, prods=[(A, V[:1]), (C, None)]),
             dict(form=2, prods=[(A13, V13), (C13, None)]), dict(form=3, prods=[(A, V[:1]), (B, W), (C, None)], frm=[-1, -1, 0])]
    for c in calls:
        plain, nt = _run(dtype, cap=cap, nt=0, **c), _run(dtype, cap=cap, nt=1, **c)
        for p, q in zip(plain, nt):
            assert (p.nt, q.nt) == (0, 1) and (p.nseg, p.grid, p.route) == (q.nseg, q.grid, q.route)
            assert _same(p.raw, q.raw) and (p.y is None or _same(p.y_raw, q.y_raw)), c["form"]
            assert not _is_fill(p.y) if p.y is not None else np.isfinite(p.rows[:, :, :p.k]).all()
    _report("nt against plain, forms 0, 2, 3", dtype, worst=0.0)


# ---------------------------------------------------------------- the batched launch


@pytest.mark.parametrize("dtype", DTYPES)
def test_batched_launch_equals_separate_launches(dtype):
    """Three products of different (m, k) in one launch: three different grids, so two of them are narrower than the launch and their
    surplus workgroups have to leave; every partial row bit-identical to three separate launches.  With the middle product's skip
    flag set its buffer keeps the pattern and the other two are unchanged.  A fourth block chained to the first goes into the second
    launch of the hook and equals form 2."""
    cap = ONE_PASS[dtype]
    shapes = [(700, 37), (_m_for(9, dtype), 121), (300, 1100)]
    prods = [_gauss(40 + i, m, k, dtype) for i, (m, k) in enumerate(shapes)]
    alone = [_run(dtype, 0, [pr], cap=cap)[0] for pr in prods]
    batch = _run(dtype, 3, prods, cap=cap)
    grids = [p.grid for p in batch]
    assert len(set(grids)) == 3 and all(p.width == max(grids) for p in batch) and [p.grid for p in alone] == grids
    assert all(p.nt == 0 and p.grid_is_consistent() for p in batch)
    worst = 0.0
    for p, q, (A, V) in zip(batch, alone, prods):
        assert (p.nseg, p.seg_len, p.route) == (q.nseg, q.seg_len, ROUTE_PLAIN) and _same(p.rows, q.rows) and p.untouched_is_fill()
        worst = max(worst, _worst_row_error(p, A, V))
    assert worst < TOL[dtype]
    skipped = _run(dtype, 3, prods, cap=cap, skip=[0, 1, 0])
    assert _is_fill(skipped[1].raw) and _same(skipped[0].raw, batch[0].raw) and _same(skipped[2].raw, batch[2].raw)
    C, _ = _gauss(44, 37, 45, dtype)
    D, _ = _gauss(45, 121, 29, dtype)
    chained = _run(dtype, 3, prods + [(C, None), (D, None)], cap=cap, frm=[-1, -1, -1, 0, 1])
    for first, last, M in ((0, 3, C), (1, 4, D)):
        a, b = _run(dtype, 2, [prods[first], (M, None)], cap=cap)
        assert chained[last].vparts == batch[first].nseg and chained[last].route == ROUTE_KERNEL
        assert _same(chained[first].rows, a.rows) and b.nseg == 1 and chained[last].width == max(chained[3].grid, chained[4].grid)
        assert _same(chained[last].rows[0, 0, :b.k], b.y)          # (form 2 took the one-segment shortcut: its row is y)
    _report("form 3 batch", dtype, worst=worst, grids=grids, width=max(grids))


# ---------------------------------------------------------------- skip


@pytest.mark.parametrize("dtype", DTYPES)
def test_skip_leaves_every_output_as_it_was(dtype):
    """The device skip flag set: forms 0, 1 and 2 write nothing -- partial rows, y, and on the reduce route of form 2 the consumer of
    the `red` buffer (which the hook fills with the pattern too: a consumer that ran would turn it into numbers or NaN all the same)."""
    cap = ONE_PASS[dtype]
    A, V = _gauss(60, _m_for(13, dtype), 300, dtype, 2)
    C, _ = _gauss(61, 300, 21, dtype)
    p, = _run(dtype, 0, [(A, V)], nrhs=2, cap=cap, skip=[1])
    assert p.nseg == 13 and _is_fill(p.raw)
    for c in (0, cap):
        p, = _run(dtype, 1, [(np.asfortranarray(A[:300]), V[:1, :300].copy())], cap=c, skip=[1])
        assert (p.nseg == 1) == (c == 0) and _is_fill(p.raw) and _is_fill(p.y_raw)      # the one-segment shortcut, and rows + reduce
    a, b = _run(dtype, 2, [(A, V[:1]), (C, None)], cap=cap, skip=[1, 1])
    assert (a.nseg, b.route) == (13, ROUTE_REDUCE) and _is_fill(a.raw) and _is_fill(b.raw) and _is_fill(b.y_raw)
    a, b = _run(dtype, 2, [(A, V[:1]), (C, None)], cap=cap, skip=[0, 1])
    f, = _run(dtype, 0, [(A, V[:1])], cap=cap)
    assert _same(a.rows, f.rows) and a.untouched_is_fill() and _is_fill(b.raw) and _is_fill(b.y_raw)
    A9, V9 = _gauss(62, _m_for(9, dtype), 300, dtype)
    a, b = _run(dtype, 2, [(A9, V9), (C, None)], cap=cap, skip=[1, 1])
    assert (a.nseg, b.route) == (9, ROUTE_KERNEL) and _is_fill(a.raw) and _is_fill(b.raw) and _is_fill(b.y_raw)


# ---------------------------------------------------------------- big64


def test_big64_plan_of_the_c5_shapes():
    """fp64, m = k = 4100: 134.5 MB, beyond kGemvNtBytes with both dimensions above 4096, so GemvT::init itself takes 2048-row
    segments and non-temporal loads here (the smallest square shape that does is 4097 x 4097).  The same cap passed explicitly gives
    the same plan and the same bits; three partial rows against float64, and a chain out of them."""
    dtype, m = np.float64, 4100
    A, V = _gauss(77, m, m, dtype)
    own, = _run(dtype, 1, [(A, V)], rows=3)
    capped, = _run(dtype, 1, [(A, V)], cap=2048)
    assert (own.nseg, own.seg_len, own.nt) == (3, 1376, 1) == (capped.nseg, capped.seg_len, capped.nt) == _plan(m, dtype, 1, 2048) + (1,)
    assert own.grid == capped.grid and own.grid_is_consistent()
    assert _same(own.raw, capped.raw) and _same(own.y_raw, capped.y_raw) and own.untouched_is_fill()
    err = _worst_row_error(own, A, V)
    assert err < TOL[dtype] and _same(own.y, _sum_rows(own.rows[0])[:m])
    ref = A.T @ V[0]
    assert np.abs(own.y - ref).max() / (np.abs(A).T @ np.abs(V[0])).max() < TOL[dtype]
    C, _ = _gauss(78, m, 33, dtype)
    a, b = _run(dtype, 2, [(A, V), (C, None)], rows=3)
    assert (a.nseg, b.nseg, b.vparts, b.route, a.nt, b.nt) == (3, 1, 3, ROUTE_KERNEL, 1, 0) and _same(a.rows, own.rows)
    refc, scale = C.T @ ref, (np.abs(C).T @ (np.abs(A).T @ np.abs(V[0]))).max()
    errc = float(np.abs(b.y - refc).max() / scale)
    assert errc < TOL[dtype]
    _report("form 1 big64 4100 x 4100", dtype, worst=err, chain=errc, nseg=own.nseg, seg_len=own.seg_len, grid=own.grid, nt=own.nt)


# ---------------------------------------------------------------- the Gram-free operator of the wide solver

WIDE_N, WIDE_P = (1, 3, 257, 1023, 1025, 2050), (1, 3, 511, 513, 1030)


def _wide_op(X, v):
    from admm_amd import _lib
    fp = ctypes.POINTER(ctypes.c_float)
    w = np.full(X.shape[0], np.nan, np.float32)
    _lib.check(_lib.load().admm_hip_test_wide_op(X.ctypes.data_as(fp), X.shape[0], X.shape[1], v.ctypes.data_as(fp), w.ctypes.data_as(fp)))
    return w


def _wide_gauss(n, p):
    rng = np.random.default_rng(3 * n + p)
    return np.asfortranarray(rng.standard_normal((n, p)).astype(np.float32)), rng.standard_normal(n).astype(np.float32)


def test_wide_op_against_float64():
    """w = X (X'v): rows around the float4 (n % 4) and the 1024-row tile of gemv_n_partial_kernel, columns around its unrolled
    four (p % 4) and its 512-column chunk.  Gaussian data: twice the single product's tolerance of max(|X| (|X|'|v|))."""
    worst = 0.0
    for n in WIDE_N:
        for p in WIDE_P:
            X, v = _wide_gauss(n, p)
            w = _wide_op(X, v)
            X64, v64 = X.astype(np.float64), v.astype(np.float64)
            ref, scale = X64 @ (X64.T @ v64), (np.abs(X64) @ (np.abs(X64).T @ np.abs(v64))).max()
            err = float(np.abs(w - ref).max() / scale)
            assert err < 2 * TOL[np.float32], (n, p, err)
            worst = max(worst, err)
    _report("wide op gaussian", np.float32, worst=worst)


def test_wide_op_small_integers_are_exact():
    """X in {-1, 0, 1}, v in -3 .. 3: |X| (|X|'|v|) stays below 2^24 (asserted), so every sum is exact in any order and w has to
    EQUAL the int64 product: a lost tail column or a mis-tiled row cannot hide in a tolerance."""
    for n in WIDE_N:
        for p in WIDE_P:
            rng = np.random.default_rng(5 * n + p)
            Xi = rng.integers(-1, 2, size=(n, p)).astype(np.int64)
            vi = rng.integers(-3, 4, size=n).astype(np.int64)
            assert (np.abs(Xi) @ (np.abs(Xi).T @ np.abs(vi))).max() < 2 ** 24
            w = _wide_op(np.asfortranarray(Xi.astype(np.float32)), vi.astype(np.float32))
            assert np.array_equal(w.astype(np.int64), Xi @ (Xi.T @ vi)), (n, p)
