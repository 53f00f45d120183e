"""The exact 29-bit record format of the packed x-update stream (admm_amd/csrc/symv_pack.h) without a GPU, through the host hook
admm_hip_test_symv_pack_host, which encodes and decodes arrays of bit patterns with the code the pack kernel and the streaming kernel share.

Round trip: every entry either comes back with its 32 bits, or is reported as an escape with its bits in the list and +0.0 in its place.
Layout pin: a NumPy restatement of the record and of the piece-major image of a wave's chunk, compared with the hook's bytes."""
import ctypes
import os
import re

import numpy as np

INVALID_ARG = 1
_up = ctypes.POINTER(ctypes.c_uint)
CHUNK_DWORDS = 64 * 29
WINDOW = 14


def _L():
    from admm_amd import _lib
    return _lib


def _pack(bits, base=-1, cap=None):
    """bits: uint32 [nchunks][64][32] -> (base used, image [nchunks][1856], escapes [(where, bits)], escapes met, decoded like bits)."""
    L = _L()
    bits = np.ascontiguousarray(bits, dtype=np.uint32)
    nch = bits.shape[0]
    assert bits.shape == (nch, 64, 32)
    cap = bits.size if cap is None else cap
    image = np.full((nch, CHUNK_DWORDS), 0xDEADBEEF, np.uint32)
    esc = np.zeros((max(cap, 1), 2), np.uint32)
    dec = np.full(bits.shape, 0xDEADBEEF, np.uint32)
    b, met = ctypes.c_int(base), ctypes.c_longlong(-1)
    L.check(L.load().admm_hip_test_symv_pack_host(bits.ctypes.data_as(_up), nch, ctypes.byref(b), image.ctypes.data_as(_up),
                                                  esc.ctypes.data_as(_up) if cap else None, cap, ctypes.byref(met), dec.ctypes.data_as(_up)))
    return b.value, image, esc[:min(met.value, cap)], met.value, dec


def _fill(values, rng=None):
    """Whole chunks from a flat list of patterns (padded with +0.0), in the order given."""
    v = np.asarray(values, dtype=np.uint32).ravel()
    n = -(-v.size // 2048) * 2048
    out = np.zeros(n, np.uint32)
    out[:v.size] = v
    return out.reshape(-1, 64, 32)


def _fits(bits, base):
    """The format's rule, restated: zero, or finite with the upper seven exponent bits in base - 13 .. base."""
    bits = bits.astype(np.uint64)
    mag = bits & 0x7FFFFFFF
    e8 = (bits >> 23) & 0xFF
    d = base - ((bits >> 24) & 0x7F).astype(np.int64)
    return (mag == 0) | ((e8 != 255) & (d >= 0) & (d < WINDOW))


def _check_round_trip(bits, base):
    used, image, esc, met, dec = _pack(bits, base)
    assert used == base
    fits = _fits(bits, base)
    assert np.array_equal(dec[fits], bits[fits])                        # exactly the 32 bits
    assert (dec[~fits] == 0).all()                                      # +0.0 in the place of an escape
    assert met == int((~fits).sum()) == len(esc)
    where = esc[:, 0].astype(np.int64)
    listed = np.zeros(bits.shape, bool)
    listed[where >> 11, (where >> 5) & 63, where & 31] = True
    assert np.array_equal(listed, ~fits)                                # every escape once, nothing else
    assert np.array_equal(bits[where >> 11, (where >> 5) & 63, where & 31], esc[:, 1])      # with its bits
    return image


def test_every_sign_and_exponent_against_several_bases():
    rng = np.random.default_rng(29)
    mant = np.concatenate([[0, 0x7FFFFF, 1, 0x400000], rng.integers(0, 1 << 23, size=12)]).astype(np.uint32)
    exps = np.arange(256, dtype=np.uint32)
    pats = ((exps[:, None] << 23) | mant[None, :]).ravel()
    pats = np.concatenate([pats, pats | 0x80000000])                    # every exponent field, both signs: +-0, denormals, +-inf, NaNs among them
    for base in (0, 1, 5, 13, 14, 20, 57, 63, 64, 100, 126, 127):
        _check_round_trip(_fill(pats), base)


def test_the_edges_of_the_window_and_one_step_outside():
    for base in (13, 14, 40, 63, 127):
        pats = []
        for e7 in (base + 1, base, base - 13, base - 14):              # one above, the two edges, one below
            if 0 <= e7 <= 127:
                for low in (0, 1):                                      # the lowest exponent bit
                    for m in (0, 0x7FFFFF, 0x2AAAAA):
                        for s in (0, 1):
                            pats.append((s << 31) | (e7 << 24) | (low << 23) | m)
        bits = _fill(pats)
        _check_round_trip(bits, base)
        fits = _fits(np.asarray(pats, np.uint32), base)
        e7s = (np.asarray(pats, np.uint64) >> 24) & 0x7F
        nonfinite = ((np.asarray(pats, np.uint64) >> 23) & 0xFF) == 255
        zero = (np.asarray(pats, np.uint64) & 0x7FFFFFFF) == 0           # base 13 / 14: the step below the window holds +-0, which has a code of its own
        assert np.array_equal(fits, zero | ((e7s <= base) & (e7s >= base - 13) & ~nonfinite))


def test_special_values_and_random_mantissas():
    rng = np.random.default_rng(5)
    special = [0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00400000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001]
    base = 60
    rnd = ((rng.integers(0, 2, size=6000, dtype=np.uint64) << 31) | (rng.integers(base - 16, base + 2, size=6000, dtype=np.uint64) << 24)
           | rng.integers(0, 1 << 24, size=6000, dtype=np.uint64)).astype(np.uint32)
    ones = np.asarray([(base - 3) << 24, ((base - 3) << 24) | 0xFFFFFF, 0x80000000 | ((base - 13) << 24) | 0xFFFFFF], np.uint32)
    bits = _fill(np.concatenate([np.asarray(special, np.uint32), ones, rnd]))
    _check_round_trip(bits, base)
    # a denormal inside the window of a small base comes back exactly, no escape
    used, _, esc, met, dec = _pack(_fill([0x00000001, 0x807FFFFF, 0x00800000, 0x0C000000]), -1)
    assert used == 12 and met == 0 and dec.ravel()[:4].tolist() == [0x00000001, 0x807FFFFF, 0x00800000, 0x0C000000]


def test_the_base_is_the_largest_finite_nonzero_exponent():
    bits = _fill([0x3F800000, 0x7F800000, 0x7FC00000, 0x00000000, 0x42000000, 0xC1000000])      # 1.0, inf, NaN, 0, 32.0, -8.0
    used, _, esc, met, dec = _pack(bits, -1)
    assert used == 0x42 and met == 2
    assert sorted(esc[:, 1].tolist()) == [0x7F800000, 0x7FC00000]


def test_escapes_beyond_the_capacity_are_counted_not_stored():
    bits = _fill([0x7FC00000 + k for k in range(40)] + [0x3F800000])
    _, _, esc, met, _ = _pack(bits, -1, cap=8)
    assert met == 40 and len(esc) == 8
    _, _, esc, met, _ = _pack(bits, -1, cap=0)
    assert met == 40 and len(esc) == 0


def _numpy_image(bits, base):
    """The record layout, restated.  Entry e = 4 k + c of a lane (column k, component c).  Record dwords 0 .. 3: the d fields (entry
    (k, c) in dword k >> 1, nibble 2 c + (k & 1)); 4 + 3 k .. 6 + 3 k: the four low-24 fields of column k as a 96-bit little-endian
    string; 28: the sign bits (entry (k, c) in bit 8 c + 7 - k).  Image of a chunk: 16-byte piece i of lane l at dword (64 i + l) * 4,
    dword 28 of lane l at dword 1792 + l."""
    nch = bits.shape[0]
    b = bits.astype(np.uint64)
    mag, e8 = b & 0x7FFFFFFF, (b >> 23) & 0xFF
    d = base - ((b >> 24) & 0x7F).astype(np.int64)
    zero = mag == 0
    esc = ~zero & ((e8 == 255) | (d < 0) | (d >= WINDOW))
    code = np.where(zero, 14, np.where(esc, 15, d)).astype(np.uint64)
    sign = np.where(esc, 0, b >> 31).astype(np.uint64)
    low = np.where(zero | esc, 0, b & 0xFFFFFF).astype(np.uint64)
    rec = np.zeros((nch, 64, 29), np.uint64)
    for e in range(32):
        k, c = e >> 2, e & 3
        rec[:, :, k >> 1] |= code[:, :, e] << np.uint64(4 * (2 * c + (k & 1)))
        rec[:, :, 28] |= sign[:, :, e] << np.uint64(8 * c + 7 - k)
    for k in range(8):
        s96 = [low[:, :, 4 * k + c] for c in range(4)]
        rec[:, :, 4 + 3 * k] = (s96[0] | (s96[1] << 24)) & 0xFFFFFFFF
        rec[:, :, 5 + 3 * k] = ((s96[1] >> 8) | (s96[2] << 16)) & 0xFFFFFFFF
        rec[:, :, 6 + 3 * k] = ((s96[2] >> 16) | (s96[3] << 8)) & 0xFFFFFFFF
    image = np.zeros((nch, CHUNK_DWORDS), np.uint32)
    for lane in range(64):
        for j in range(28):
            image[:, ((j >> 2) * 64 + lane) * 4 + (j & 3)] = rec[:, lane, j]
        image[:, 1792 + lane] = rec[:, lane, 28]
    return image


def test_the_layout_is_pinned_bit_by_bit():
    rng = np.random.default_rng(7)
    base = 62
    bits = ((rng.integers(0, 2, size=(3, 64, 32), dtype=np.uint64) << 31) | (rng.integers(base - 15, base + 1, size=(3, 64, 32), dtype=np.uint64) << 24)
            | rng.integers(0, 1 << 24, size=(3, 64, 32), dtype=np.uint64)).astype(np.uint32)
    bits[0, 5, 7] = 0x80000000
    bits[1, 63, 31] = 0x7FC00000
    bits[2, 0, 0] = 0
    image = _check_round_trip(bits, base)
    assert image.tobytes() == _numpy_image(bits, base).tobytes()
    assert image.nbytes == 3 * 7424                                    # 7 x 1 KiB + 256 B per chunk: 29 bits per entry
    # one entry alone: lane 9, entry 22 (column 5, component 2), negative, d = 3, low 24 bits 0xABCDEF
    one = np.zeros((1, 64, 32), np.uint32)
    one[0, 9, 22] = 0x80000000 | ((base - 3) << 24) | 0xABCDEF
    _, img, _, met, _ = _pack(one, base)
    want = np.zeros(CHUNK_DWORDS, np.uint32)
    for lane in range(64):                                             # zeros are d = 14 in every nibble
        for j in range(4):
            want[(0 * 64 + lane) * 4 + j] = 0xEEEEEEEE
    want[9 * 4 + 2] = 0xEE3EEEEE                                       # column 5, component 2: dword 2 of the record, nibble 2 * 2 + 1
    # low field of column 5, component 2: bits 48 .. 71 of the 96-bit string in record dwords 19, 20, 21 = pieces 4 (dword 3) and 5 (dwords 0, 1)
    want[(4 * 64 + 9) * 4 + 3] = 0
    want[(5 * 64 + 9) * 4 + 0] = (0xABCDEF << 16) & 0xFFFFFFFF
    want[(5 * 64 + 9) * 4 + 1] = 0xABCDEF >> 16
    want[1792 + 9] = 1 << (8 * 2 + 7 - 5)
    assert met == 0 and np.array_equal(img[0], want)


def test_the_hooks_are_declared_exported_bound_and_listed():
    L = _L()
    lib = L.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "admm_hip.h")).read(), flags=re.S)
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    for sym, nargs in (("admm_hip_test_symv_pack_host", 8), ("admm_hip_test_symv_packed", 14), ("admm_hip_test_symv_packed_time", 6),
                       ("admm_hip_test_tall_pack_info", 1)):
        assert re.search(r"\b%s\s*\(" % sym, hdr)
        assert hasattr(lib, sym) and sym in L.EXPORTS
        assert len(getattr(lib, sym).argtypes) == nargs and getattr(lib, sym).restype is ctypes.c_int
        assert "`%s`" % sym in doc


def test_the_hooks_refuse_bad_arguments_before_they_look_for_a_device():
    lib = _L().load()
    bits = np.zeros((1, 64, 32), np.uint32)
    out = np.zeros(CHUNK_DWORDS, np.uint32)
    b, met = ctypes.c_int(0), ctypes.c_longlong()
    p = lambda a: a.ctypes.data_as(_up)
    assert lib.admm_hip_test_symv_pack_host(None, 1, ctypes.byref(b), p(out), None, 0, ctypes.byref(met), p(bits)) == INVALID_ARG
    assert lib.admm_hip_test_symv_pack_host(p(bits), 0, ctypes.byref(b), p(out), None, 0, ctypes.byref(met), p(bits)) == INVALID_ARG
    assert lib.admm_hip_test_symv_pack_host(p(bits), 1, ctypes.byref(b), p(out), None, 4, ctypes.byref(met), p(bits)) == INVALID_ARG
    assert "symv_pack_host hook" in lib.admm_hip_last_error().decode()
    fp = ctypes.POINTER(ctypes.c_float)
    A = np.eye(5, dtype=np.float32, order="F")
    v = np.ones(5, np.float32)
    y = np.zeros((2, 5), np.float32)
    info, so = (ctypes.c_longlong * 8)(), (ctypes.c_int * 3)()
    f = lambda a: a.ctypes.data_as(fp)
    for gate, nt, cap, pp in ((3, 0, 32, 5), (0, 2, 32, 5), (0, 0, -1, 5), (0, 0, 32, 0), (0, 0, 32, 32769)):
        assert lib.admm_hip_test_symv_packed(f(A), pp, f(v), f(v), gate, nt, 0, cap, f(y), None, None, 0, info, so) == INVALID_ARG
        assert "symv_packed hook" in lib.admm_hip_last_error().decode()
    us = np.zeros((4, 2), np.float32)
    assert lib.admm_hip_test_symv_packed_time(f(A), 5, f(v), 3, f(us), info) == INVALID_ARG
    assert "symv_packed_time hook" in lib.admm_hip_last_error().decode()
