// The exact 29-bit storage of the cached inverse for the tall x-update's one-vector kernel (symv_kernels.h: symv1_packed_kernel).
// One copy of the format, shared by the pack kernel, the streaming kernel and the host hook admm_hip_test_symv_pack_host.
//
// The entries of one tile lie in a narrow band of exponents.  With `base` = the largest value of the upper SEVEN exponent bits
// (bits 30 .. 24) among the finite non-zero entries of the tile, an entry whose upper seven exponent bits are base - d, d = 0 .. 13,
// is its sign, the 4-bit d and its low 24 bits (the lowest exponent bit and the 23 mantissa bits): 29 bits, from which the 32 come
// back exactly.  d = 14: +-0.0 with that sign.  d = 15: escape -- the record holds +0.0 in that place and the whole float stands in
// the tile's escape list.  Non-finite values and everything outside the window are escapes.
//
// Record = one lane's share of one 8-column chunk of a tile: 4 rows x 8 columns = 32 entries, entry (k, c) = column k of the chunk,
// component c of the lane's float4 (e = 4 k + c where entries are numbered) = 29 dwords:
//   dwords 0 .. 3     the 32 d fields: entry (k, c) in dword k >> 1, nibble 2 c + (k & 1) -- the four fields of a column are the low
//                     nibbles (even k) or the high nibbles (odd k) of the four bytes of their dword
//   dwords 4 .. 27    the 32 low-24 fields: column k in dwords 4 + 3 k .. 6 + 3 k as a 96-bit little-endian string of its four fields
//   dword 28          the 32 sign bits: entry (k, c) in bit 8 c + 7 - k -- shifted left by k, the four signs of column k are the top
//                     bits of the four bytes
// so that the four top bytes of a column (sign, upper seven exponent bits) are formed together, byte-wise in one register, and each
// entry is then one or two byte permutes (sp_column_decode).
// In memory the 64 records of a wave's chunk are stored piece-major: piece i (i = 0 .. 6) of lane l = dwords 4 i .. 4 i + 3 of its
// record at dword (64 i + l) * 4 of the chunk, dword 28 of lane l at dword 1792 + l.  A chunk is 7 x 1 KiB + 256 B = 7424 contiguous
// bytes (58 lines of 128), fetched by a wave with seven 16-byte requests and one 4-byte request per lane.  The chunks of a wave, the
// waves of a tile and the tiles of a plan follow one another in the order the kernel walks them.
#pragma once
#include <hip/hip_runtime.h>

namespace admm {

constexpr int kSpEntries = 32;                         // entries of a record
constexpr int kSpRecDwords = 29;
constexpr int kSpPieces = 7;                           // 16-byte pieces of a record (the 4-byte piece follows them)
constexpr int kSpChunkDwords = 64 * kSpRecDwords;      // a wave's chunk: 1856 dwords
constexpr int kSpChunkBytes = kSpChunkDwords * 4;      // 7424
constexpr unsigned kSpWindow = 14;                     // d = 0 .. 13 are exponents
constexpr unsigned kSpZero = 14, kSpEscape = 15;
constexpr int kSpEscCap = 32;                          // default capacity of a tile's escape list
static_assert(kSpChunkBytes % 128 == 0, "a wave's chunk is whole 128-byte lines");

__host__ __device__ inline int sp_exp7(unsigned bits) { return (int)((bits >> 24) & 0x7Fu); }
// does the entry take part in its tile's base: finite and not a zero
__host__ __device__ inline bool sp_counts(unsigned bits) { return (bits & 0x7FFFFFFFu) != 0u && ((bits >> 23) & 0xFFu) != 0xFFu; }
// the 5-bit code (sign << 4 | d) of a float's bits against a tile's base
__host__ __device__ inline unsigned sp_code(unsigned bits, int base) {
    if ((bits & 0x7FFFFFFFu) == 0u) return ((bits >> 31) << 4) | kSpZero;
    if (((bits >> 23) & 0xFFu) == 0xFFu) return kSpEscape;
    const int d = base - sp_exp7(bits);
    if (d < 0 || d >= (int)kSpWindow) return kSpEscape;
    return ((bits >> 31) << 4) | (unsigned)d;
}
__host__ __device__ inline unsigned sp_low24(unsigned bits, unsigned code) { return (code & 15u) >= kSpZero ? 0u : (bits & 0xFFFFFFu); }
// dword of a wave's chunk that holds dword j of lane l's record
__host__ __device__ inline int sp_dword_pos(int lane, int j) { return j < 4 * kSpPieces ? ((j >> 2) * 64 + lane) * 4 + (j & 3) : 4 * kSpPieces * 64 + lane; }
__host__ __device__ inline int sp_d_shift(int k, int c) { return 4 * (2 * c + (k & 1)); }      // within dword k >> 1
__host__ __device__ inline int sp_sign_bit(int k, int c) { return 8 * c + 7 - k; }              // within dword 28

// 32 floats (as bits, entry 4 k + c) -> record; bit 4 k + c of the returned mask: that entry is an escape (its place holds +0.0, the
// caller lists the float)
__host__ __device__ inline unsigned sp_record_encode(const unsigned (&bits)[kSpEntries], int base, unsigned (&rec)[kSpRecDwords]) {
    unsigned esc = 0u, signs = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) rec[j] = 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        unsigned lo[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int e = 4 * k + c;
            const unsigned code = sp_code(bits[e], base);
            if (code == kSpEscape) esc |= 1u << e;
            signs |= (code >> 4) << sp_sign_bit(k, c);
            rec[k >> 1] |= (code & 15u) << sp_d_shift(k, c);
            lo[c] = sp_low24(bits[e], code);
        }
        rec[4 + 3 * k] = lo[0] | (lo[1] << 24);
        rec[5 + 3 * k] = (lo[1] >> 8) | (lo[2] << 16);
        rec[6 + 3 * k] = (lo[2] >> 16) | (lo[3] << 8);
    }
    rec[28] = signs;
    return esc;
}

// Entry by entry, as the format is stated: the reference the host hook holds sp_column_decode against (and the dev build
// ADMM_HIP_SYMV_PACK_DEC=1 of the streaming kernel).  Escapes come back as +0.0.
__host__ __device__ inline void sp_column_decode_plain(unsigned dsel, unsigned w0, unsigned w1, unsigned w2, unsigned signs, int k, int base, unsigned (&out)[4]) {
    const unsigned lo[4] = {w0 & 0xFFFFFFu, ((w0 >> 24) | (w1 << 8)) & 0xFFFFFFu, ((w1 >> 16) | (w2 << 16)) & 0xFFFFFFu, w2 >> 8};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const unsigned d = (dsel >> sp_d_shift(k, c)) & 15u;
        const unsigned top = d >= kSpZero ? 0u : (unsigned)base - d;
        out[c] = (((signs >> sp_sign_bit(k, c)) & 1u) << 31) | (top << 24) | lo[c];
    }
}

// v_perm_b32: byte i of the result is byte sel_i (0 .. 7) of the eight bytes {hi, lo}, lo = bytes 0 .. 3
__host__ __device__ inline unsigned sp_perm(unsigned hi, unsigned lo, unsigned sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const unsigned long long both = ((unsigned long long)hi << 32) | lo;
    unsigned r = 0u;
    for (int i = 0; i < 4; ++i) r |= (unsigned)((both >> (8 * ((sel >> (8 * i)) & 7u))) & 0xFFu) << (8 * i);
    return r;
#endif
}

// Column k of a record: its d dword (dword k >> 1), its three low dwords, the sign dword -> the four floats (as bits).  The four top bytes
// are formed byte-wise in one register: base - d under a guard bit (no borrow between the bytes), zeroed where d >= 14, the sign bits in.
__host__ __device__ inline void sp_column_decode(unsigned dsel, unsigned w0, unsigned w1, unsigned w2, unsigned signs, int k, int base, unsigned (&out)[4]) {
    const unsigned d4 = (dsel >> (4 * (k & 1))) & 0x0F0F0F0Fu;
    const unsigned z = (d4 + 0x02020202u) & 0x10101010u;               // bit 4 of a byte: d >= 14
    const unsigned gone = (z << 4) - (z >> 4);                         // 0xFF in those bytes
    const unsigned b4 = (unsigned)base * 0x01010101u | 0x80808080u;
    const unsigned x = (b4 - d4) & ~gone;
    const unsigned t4 = (x & 0x7F7F7F7Fu) | ((signs << k) & 0x80808080u);
    out[0] = sp_perm(t4, w0, 0x04020100u);
    out[1] = sp_perm(t4, sp_perm(w1, w0, 0x00050403u), 0x05020100u);
    out[2] = sp_perm(t4, sp_perm(w2, w1, 0x00040302u), 0x06020100u);
    out[3] = sp_perm(t4, w2, 0x07030201u);
}

#ifndef ADMM_HIP_SYMV_PACK_DEC
#define ADMM_HIP_SYMV_PACK_DEC 0      // dev builds: 1 = the entry-by-entry decode in the streaming kernel ("Measured and rejected", symv_kernels.h)
#endif

// record -> the 32 floats (as bits); escapes come back as +0.0
__host__ __device__ inline void sp_record_decode(const unsigned (&rec)[kSpRecDwords], int base, unsigned (&out)[kSpEntries]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        unsigned o[4];
#if ADMM_HIP_SYMV_PACK_DEC == 1
        sp_column_decode_plain(rec[k >> 1], rec[4 + 3 * k], rec[5 + 3 * k], rec[6 + 3 * k], rec[28], k, base, o);
#else
        sp_column_decode(rec[k >> 1], rec[4 + 3 * k], rec[5 + 3 * k], rec[6 + 3 * k], rec[28], k, base, o);
#endif
        out[4 * k] = o[0]; out[4 * k + 1] = o[1]; out[4 * k + 2] = o[2]; out[4 * k + 3] = o[3];
    }
}

}  // namespace admm
