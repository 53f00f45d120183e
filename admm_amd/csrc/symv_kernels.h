// Symmetric mat-vec that reads only the lower triangle, for the tall x-update.
//
//   y_r = A v_r  (r = 0, 1)  for a symmetric p x p fp32 matrix stored column-major (both triangles
//   are in memory, only tiles on or below the diagonal are read): 2 p^2 bytes instead of 4 p^2.
//
// Tiling: a workgroup owns 256 rows x a column segment of its row strip (round 3: 32 .. 256 columns, SymvSched below;
// round 2: always 128); each of its 4 waves owns the same 256 rows (one float4 per lane) and a quarter of the columns.
// Measured on C2, same box (round 2, fixed widths): 128-column tiles 35.1 us per launch, 23.2 k ADMM iterations/s;
// 256-column tiles with 64 columns per wave halve the axpy partial rows (tail 6.6 instead of 7.1 us) but the longer
// per-wave column loop streams worse: 37.7 us, 22.0 k it/s; 512-column tiles leave too few workgroups: 51 us.
// Also measured and rejected (round 2): both right-hand sides as pairs through v_pk_fma_f32 plus separate loop copies for
// diagonal / interior / ragged tiles (half the FMA instructions, 32 instead of 74 selects per chunk in the hot copy):
// 36.7 us -- the loop is not VALU-bound, and the scheduling of its 8 loads in flight is what the time depends on.  For every element a_ij (i > j) it loads, a wave
// does both halves of the symmetric product:
//     dot  part:  y_j += a_ij v_i   -> per-lane partials of 8 columns at a time, combined across
//                                      the 64 lanes with a halving butterfly (10 shuffles per 8 columns)
//     axpy part:  y_i += a_ij v_j   -> 4 per-lane accumulators (v_j is wave-uniform, v_readlane)
// The diagonal element contributes once (dot part).  Results are written as partials:
//     dot[rb][j]  (rb = row block of 256)      axp[cb][i]  (cb = column block of 128)
// and summed by the consumer (`symv_sum_partials` below, fused into the tall tail kernel):
//     y_i = sum_{rb >= cb(i)/2} dot[rb][i] + sum_{cb <= 2 rb(i) + 1} axp[cb][i].
// Deterministic (no atomics).  Partial traffic: (p/256 + p/128) * p * 8 bytes per launch, written
// once and read once (about 9 % of the triangle at p = 10^4).
//
// Measured and rejected (scripts/symv_tune.hip, scripts/symv_check.hip, in-situ A/B of the tall loop):
//  * packing the triangle tile by tile (each 128 KB tile contiguous): +-2..6 % depending on p, -1 % in the
//    loop at p = 10^4;
//  * alternating the tile order between launches so that an XCD reads first what it read last (order of the groups of 8
//    tiles reversed on odd launches; a tile keeps its XCD): no change at all (24.10 vs 24.10 k it/s) -- nothing of the
//    matrix survives a kernel boundary in the XCD L2s.  In-kernel timestamps (scripts/tall_probe.py) put the streaming
//    phase itself at 200 MB / 31 us = 6.45 TB/s, the Infinity Cache ceiling; the rest of the 34.5 us is ramp and drain;
//  * 5 or 6 workgroups per CU (launch bounds) so that all 1600 tiles of p = 10^4 are resident at once and end together (the
//    probe shows ~2.6 us between the end of the last tile in the list and the true last end): 96 / 80 registers spill the
//    column chunk -- 47 / 113 us per launch;
//  * two or three tiles per workgroup (half / a third of the workgroups, same tile code): 38.1 / 38.3 instead of 35.6 us
//    per launch -- the second round of small work units is what balances the end of the launch;
//  * fusing the consumer into this launch ("last tile of a block finalises it", arrival counters): correct,
//    but cross-XCD visibility needs either agent-scope fences (whole-L2 write-back per wave: 5x slower) or
//    uncached partial arrays plus an acknowledged-store wait and an atomic round trip per tile (1.65x slower
//    than two launches).
// Round 7, work whose result nobody uses (profiles/r07_tall_dead_work.md; C2, same box, parent and new alternating):
//  * diagonal blocks: a lane whose four rows all lie above a column no longer loads that float4 (`last` in symv2_tile).  PMC: 202.6 MB
//    read per launch instead of 207.1 (the triangle is 200); 33.0 instead of 33.7 us per launch in the kernel trace;
//  * prologue: the `done` word, the verdict word and the tile descriptor are requested together -- one round trip before the first
//    matrix request instead of two;
//  * launches whose products are discarded (100 of the 2264 of a C2 path) end early: SymvVerdict below.  Checked in the prologue only,
//    the 636 tiles that are not resident at the start leave (63 600 per path) and such a launch takes 29.6 us; checked between
//    the chunks as well it takes 19.5 us and the path 85.8-87.8 ms against 86.9-90.1 (parent: 89.1-90.7), regular launches 33.2
//    against 33.1 us.  A first form that kept the word in vector registers through the chunk spilled (24 bytes of scratch, a reload
//    in the loop) and was not measured: the word is compared as two scalars right behind the chunk's wait.
// Round 8, the decision before the stream (profiles/tall_decide_first.md): the tall solver's default x-update is symv1_lower_kernel below --
// still two launches per iteration, but every tile takes the launch's decision itself in its prologue (a Gate functor) and multiplies ONE
// vector, or leaves.  symv2_lower_kernel stays for the verdict-word levels, the sharded and the refined paths.
// Measured and rejected there (C2, same box, kernel trace of parent and variants in one session):
//  * 5 or 6 workgroups per CU for the one-vector kernel (ADMM_HIP_SYMV1_WGS): it needs 117 VGPRs at 4; bounded to 96 / 80 it spills the
//    column chunk like the two-vector kernel did (124-128 / 188 bytes of scratch per lane, with or without the peeled first chunk):
//    not measured, 4 kept;
//  * the gate evaluated BEFORE the first matrix request (ADMM_HIP_SYMV1_PRE=0: no peeled chunk, a leaving tile requests nothing):
//    regular launches 34.6 us against 32.9 with the first chunk requested ahead of the gate (two-vector kernel: 32.9) -- the block sum
//    and its two barriers are exposed in every tile; 89.9-90.1 ms per path against 87.0-87.8;
//  * the gate reading the 64-byte rows of the norm partials as block 0 does (313 rows, a wave's load touching 64 lines): regular launches
//    2 us slower than the two-vector kernel's; the tails now write a compact copy (lasso_tall.hip: tall_publish_norms).
// Round 9, fewer bytes (profiles/tall_packed_stream.md): symv1_packed_kernel streams an exact 29-bit copy of the tiles (symv_pack.h) and decodes
// it to the fp32 matrix's bits in front of symv1_tile's one copy of the arithmetic; the tall solver's default where it runs symv1_lower_kernel.
// The bare tile loops, p = 10^4, replayed back to back (C2's box type, event-timed, medians of 20 launches, two sessions of each):
//   fp32 31.0 - 32.6 us | packed 29.6 - 29.9 us | the 29 dwords consumed undecoded (the floor of this stream) 29.0 - 29.4 us.
// Measured and rejected there:
//  * the decode entry by entry (extract d, subtract, compare and select for the zero code, shift and or: 646 vector and 294 scalar
//    instructions in the column loop against the fp32 kernel's 298 and 134): 31.7 - 31.9 us, no faster than the fp32 stream -- the loop
//    then IS bound by its instructions.  The format's code bits are therefore laid out so that the four top bytes of a column are formed
//    byte-wise in one register and every entry is one or two v_perm_b32 (about 420 vector instructions on the path without escapes, 99 VGPRs): within 0.6 us of the floor;
//  * the floor itself is 2 us under the fp32 stream, not the 2.9 us the byte ratio promises: a chunk is still eight requests per lane.
// Round 10, a second chunk in flight per wave (profiles/tall_two_chunks.md): the packed kernel's column loop requests chunk q + 1 into a second
// record buffer before it decodes chunk q (SymvPackedSrc: ping / pong; symv1_tile: the loop unrolled by two).  What made it fit and overlap:
//  * the requests are buffer loads whose dead lanes (above the diagonal, beyond p - 1 or the last row, no chunk left) carry an offset out of
//    the descriptor's range -- straight-line code.  With the loads under the per-lane branch they had, the compiler's wait counts cover the
//    path that skipped them, and the decode of chunk q waited for chunk q + 1 as well (s_waitcnt vmcnt(0) behind the request ahead);
//  * the wave's number is a scalar (readfirstlane): first column, chunk count and the descriptor are scalars, 128 VGPRs and 8 - 12 bytes of
//    scratch became 124 and none (4 waves per SIMD).  One chunk deep the same source needs 92 VGPRs (99 before) and runs 5 workgroups per CU.
// Bare tile loops, p = 10^4, replayed back to back, three builds in one process, medians of 3 x 20 launches, two sessions: parent 31.10 /
// 30.84 us | two chunks at 4 workgroups per CU (kept) 30.68 / 30.40 | one chunk deep at 5 (ADMM_HIP_SYMV1_DEPTH=1) 30.96 / 30.14; the fp32
// loop, the same code in all three builds, 30.6 - 31.7.  C2 path: 81.9 - 82.4 ms per step against 82.8 - 83.0 (five alternating pairs).
// Measured and not kept: the one-deep loop at 5 workgroups per CU (above: the same gain on average, less steady; not run through the
// path); not built: requesting only the first pieces of chunk q + 1 ahead (two whole chunks fit).
// Round 11, every prologue request before the first wait (profiles/tall_prologue.md; the measurements are there).  Read from the compiled
// code, not from the source: symv1_tile's "one batch" had become three serialised vector round trips (a norm-partial load, its wait and
// its add per column: the guards `w < nwg` on the load and on the add had been merged into one predicated block) and three to four
// scalar ones (kernel arguments fetched as first used; the descriptor, the packed descriptor and the gate's control block sunk below the
// `done` branch) in front of the first matrix byte, and the one-plane tail was two round trips (element loads, a wait, then the partials:
// the address of the first partial read a register pair whose upper half was a pending load's destination).  Now, in the four default
// instantiations: kernel arguments, one lgkmcnt(0); the batch -- six branch-free norm-partial loads (lasso_tall.hip), the tile descriptor,
// `done`, the control block, the packed descriptor -- one lgkmcnt(0); chunk 0; the gate's first use of a norm partial at vmcnt(13), i.e.
// behind nothing but its own loads.  What holds the order: a scheduling barrier above the batch, a compiler-level memory fence and pins
// of the kernel arguments below it (a pin ABOVE the batch turned the control words' scalar loads into vector loads), the packed source's
// chunk-0 request without its branch, and the tail's partial requests ahead of its element loads (symv_sum_partials1: `behind`).
// tests/test_tall_prologue_asm.py reads the order from the assembly.  Same addends, same order, same block_sum: no result moves.
// Not built: the row and column entries of both candidate vectors requested with chunk 0 (5 + 5 more live VGPRs at 124 of 128).
#pragma once
#include "admm_internal.h"
#include "device_utils.h"
#include "symv_pack.h"
#include <hip/hip_ext.h>
#include <climits>
#include <type_traits>

namespace admm {

constexpr int kSyRB = 256;     // rows per tile
constexpr int kSyCB = 128;     // default columns per workgroup tile (round 2's fixed tile)
constexpr int kSyCBMax = 256;  // widest column segment a workgroup may own (64 columns per wave: one register of right-hand entries)
static_assert(kSyCBMax == 256, "SYMV_SCHED's widths are checked against 256 where the option is parsed (options.hip)");
constexpr int kSyThreads = 256;

// Round 3: a tile is 256 rows x a column SEGMENT [c0, c0 + width) of its row strip, width a multiple of 32 up to kSyCBMax,
// each of the 4 waves owning width / 4 consecutive columns.  The strips are cut with one of two widths (SymvSched): the
// long strips, dispatched first, in wide segments; the short strips, dispatched last, in narrow ones -- the end of the
// launch is then made of small work units (the integer number of tiles a CU gets no longer leaves some CUs a whole
// 256 x 128 tile short of the others), and the wide segments leave fewer axpy partial rows for the consumer to sum.
// width_big = width_small = 128 reproduces round 2's tiling and partial layout exactly.
struct SymvSched {
    int width_big = kSyCB, width_small = kSyCB;
    int rb_split = 0;              // strips rb >= rb_split are cut in width_big, the others in width_small
    __host__ __device__ int width(int rb) const { return rb >= rb_split ? width_big : width_small; }
    // segments of strip rb: its columns 0 .. min((rb + 1) * 256, p32) - 1 in pieces of width(rb)   (p32 = p rounded up to 32)
    __host__ __device__ int nseg(int rb, int p32) const {
        const int cols = min((rb + 1) * kSyRB, p32), w = width(rb);
        return (cols + w - 1) / w;
    }
};
constexpr int kSySumLanes = 8;  // lanes that share one element when the consumer sums the partials (symv_sum_partials)

struct SymvArgs {
    const float* A; long long lda; int p;
    const float* v0; const float* v1;      // right-hand vectors, allocated (and zero padded) to a multiple of 256
    float* dot0; float* dot1;              // [nrb][ldo]
    float* axp0; float* axp1;              // [ncb][ldo]
    long long ldo;
    const int4* tiles;                     // (row block, first column, width, segment index within the strip) of every tile
    const int* skip;                       // sticky `done` word (a caller without one gets the plan's zero word: never null in the kernel)
    const unsigned long long* verdict;     // kSyVerdictReplicas copies of the verdict word, one per 128-byte line (SymvVerdict below; never null in the kernel)
    unsigned long long discard;            // the one value of that word that says "the products of this launch are not used"
    unsigned long long* early;             // count of the tiles that left on it (added to on the exit path only); symv1_lower_kernel: kSyEarlySlots counters
#ifdef ADMM_HIP_PROBE
    long long* probe; int probe_idx;       // dev build only (probe.h): entry / end stamps of the first, middle and last tile
#endif
};

// Early exit of the tiles of a launch whose products nobody reads (tall solver, lasso_tall.hip: after a converged lambda the tail keeps
// the stored x, and the launch that takes the last decision of a path is not consumed at all).  The decision is taken by the extra
// workgroup of that SAME launch, so a tile can only know it if it starts late enough: the decider publishes ONE 64-bit word -- the
// run, the number of the launch and the discard bit, so that no word of another launch or of an earlier run() can be mistaken for it
// -- with write-through stores into kSyVerdictReplicas copies on lines of their own, and every tile reads its copy once, in its
// prologue, with an agent-scope load (not served by this CU's L1), together with the `done` word and its tile descriptor.  The check
// never waits: a word that is not there yet, or is another launch's, means "stream as usual".  Tiles that leave write no partials: the
// slots keep what the previous launch left, nothing reads them (the tail of a discarded launch takes x from its stored copy and sums the
// partials only into values it drops), and the next consumed launch rewrites every slot first.
constexpr int kSyVerdictReplicas = 64;     // a power of two
constexpr int kSyVerdictStride = 16;       // in words: 128 bytes
struct SymvVerdict {
    const unsigned long long* words = nullptr;      // null: the launch never leaves early
    unsigned long long discard = 0;
    unsigned long long* early = nullptr;
    bool mid = false;                               // the waves also look between the chunks of their column loop (plain-load kernel only)
};

// Sum 8 per-lane values over the 64 lanes: afterwards every lane l holds the total of value (l >> 3).
template <typename T>
__device__ __forceinline__ T butterfly8(const T (&v)[8], int lane) {
    T a4[4], a2[2];
    {
        const int b = (lane >> 5) & 1;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const T keep = b ? v[k + 4] : v[k], send = b ? v[k] : v[k + 4];
            a4[k] = keep + __shfl_xor(send, 32, 64);
        }
    }
    {
        const int b = (lane >> 4) & 1;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const T keep = b ? a4[k + 2] : a4[k], send = b ? a4[k] : a4[k + 2];
            a2[k] = keep + __shfl_xor(send, 16, 64);
        }
    }
    const int b = (lane >> 3) & 1;
    const T keep = b ? a2[1] : a2[0], send = b ? a2[0] : a2[1];
    T r = keep + __shfl_xor(send, 8, 64);
    r += __shfl_xor(r, 4, 64);
    r += __shfl_xor(r, 2, 64);
    r += __shfl_xor(r, 1, 64);
    return r;
}

// How a tile reads the right-hand vectors: ordinary loads (the vectors were written by an earlier launch).
struct SymvPlainVec {
    __device__ __forceinline__ float4 load4(const float* p) const { return *reinterpret_cast<const float4*>(p); }
    __device__ __forceinline__ float load1(const float* p) const { return *p; }
};

// One tile (kSyRB rows x kSyCB columns, 4 waves) of the symmetric product: right-hand entries first, every 8-column chunk loaded at
// the top of its loop iteration -- the shape that streams best (a first chunk requested ahead and carried into the loop in registers ran
// the same 128-column kernel at 39.3 instead of 35.1 us on C2: the carried chunk and a conditional reload defeat the scheduling of the loads).
// MID: the wave also asks for its copy of the verdict word ahead of every chunk's 8 matrix loads, reads it behind that chunk's wait and
// leaves the column loop when it says "discard" (SymvVerdict below).  The waves of a workgroup may disagree; every one still runs the
// epilogue and reaches its barrier, and what a tile that stopped half-way writes is as unread as what it would have written.
template <typename VecLoad, bool NT = false, bool MID = false>      // NT: matrix read with non-temporal loads (triangle larger than the Infinity Cache)
__device__ __forceinline__ void symv2_tile(const SymvArgs& a, const int4 t, VecLoad vl,
                                           float4 (*red)[kSyThreads], float (*sdot)[kSyCBMax]) {
    const int rb = t.x, seg = t.w;
    const int cw = t.z >> 2;               // columns per wave: a multiple of 8, at most 64
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int row = rb * kSyRB + lane * 4;
    const int col0 = t.y + wid * cw;
    const int p4 = (a.p + 3) & ~3;
    const bool active = row < p4;
    const bool has = col0 < a.p;           // every wave of a listed tile has all its columns <= the block's last row
    const float* base = a.A + (size_t)col0 * a.lda + row;
    float4 av[8];
    float4 aU = make_float4(0.f, 0.f, 0.f, 0.f), aW = aU;

    if (has) {
        const float4 uI = active ? vl.load4(a.v0 + row) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 wI = active ? vl.load4(a.v1 + row) : make_float4(0.f, 0.f, 0.f, 0.f);
        const int cj = col0 + lane;                                          // the wave's (<= 64) right-hand entries, one per lane
        const float uj = (lane < cw && cj < a.p) ? vl.load1(a.v0 + cj) : 0.f;
        const float wj = (lane < cw && cj < a.p) ? vl.load1(a.v1 + cj) : 0.f;
        const bool diag = col0 + (cw - 1) >= rb * kSyRB;         // this wave's block meets the diagonal
        const int nq = cw >> 3;
        // Last column this lane loads: p - 1, and on a wave that meets the diagonal no column beyond its last row -- there all four
        // entries of the float4 lie above the diagonal and are zeroed below whatever was loaded (about half of a 256 x 256 diagonal
        // block: 4.9 MB of whole 128-byte lines per launch at p = 10^4).  av[k] stays the zero it is initialised with, so every value
        // that enters an FMA is what it was.  One compare per column, as before (it replaces `active && col < p`).
        const int last = active ? min(a.p - 1, diag ? row + 3 : INT_MAX) : -1;
        const unsigned long long* vword = a.verdict + (size_t)(blockIdx.x & (kSyVerdictReplicas - 1)) * kSyVerdictStride;
#pragma unroll 1
        for (int q = 0; q < nq; ++q) {
            unsigned long long vq = 0;
            if constexpr (MID) vq = __hip_atomic_load(vword, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int col = col0 + q * 8 + k;
                av[k] = make_float4(0.f, 0.f, 0.f, 0.f);
                if constexpr (NT) { if (col <= last) av[k] = load16_nt<float4>(base + (size_t)(q * 8 + k) * a.lda); }
                else { if (col <= last) av[k] = *reinterpret_cast<const float4*>(base + (size_t)(q * 8 + k) * a.lda); }
            }
            if constexpr (MID) {      // the word was requested first, so it is there before the chunk is: no wait of its own.  Wave-uniform (one address), compared as scalars
                const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)vq), hi = __builtin_amdgcn_readfirstlane((unsigned)(vq >> 32));
                if ((((unsigned long long)hi << 32) | lo) == a.discard) break;
            }
            float dU[8], dW[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int col = col0 + q * 8 + k;
                float4 v = av[k];
                float4 ax = v;                                    // axpy part excludes the diagonal
                if (diag) {
                    if (row + 0 < col) v.x = 0.f;
                    if (row + 1 < col) v.y = 0.f;
                    if (row + 2 < col) v.z = 0.f;
                    if (row + 3 < col) v.w = 0.f;
                    ax = v;
                    if (row + 0 == col) ax.x = 0.f;
                    if (row + 1 == col) ax.y = 0.f;
                    if (row + 2 == col) ax.z = 0.f;
                    if (row + 3 == col) ax.w = 0.f;
                }
                dU[k] = fmaf(v.x, uI.x, fmaf(v.y, uI.y, fmaf(v.z, uI.z, v.w * uI.w)));
                dW[k] = fmaf(v.x, wI.x, fmaf(v.y, wI.y, fmaf(v.z, wI.z, v.w * wI.w)));
                const float ujc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(uj), (q * 8 + k) & 63));
                const float wjc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wj), (q * 8 + k) & 63));
                aU.x = fmaf(ax.x, ujc, aU.x); aU.y = fmaf(ax.y, ujc, aU.y); aU.z = fmaf(ax.z, ujc, aU.z); aU.w = fmaf(ax.w, ujc, aU.w);
                aW.x = fmaf(ax.x, wjc, aW.x); aW.y = fmaf(ax.y, wjc, aW.y); aW.z = fmaf(ax.z, wjc, aW.z); aW.w = fmaf(ax.w, wjc, aW.w);
            }
            // dot part of these 8 columns: every lane ends with column (lane >> 3)
            const float du = butterfly8(dU, lane);
            const float dw = butterfly8(dW, lane);
            if ((lane & 7) == 0) {
                sdot[0][wid * cw + q * 8 + (lane >> 3)] = du;
                sdot[1][wid * cw + q * 8 + (lane >> 3)] = dw;
            }
        }
    } else {
        for (int c = lane; c < cw; c += 64) { sdot[0][wid * cw + c] = 0.f; sdot[1][wid * cw + c] = 0.f; }
    }
    // axpy part: add the 4 waves (same rows, different columns); dot part: one 512-byte row per array
    red[0][threadIdx.x] = aU;
    red[1][threadIdx.x] = aW;
    __syncthreads();
    if (wid < 2) {
        float4 s = red[wid][lane];
#pragma unroll
        for (int ww = 1; ww < 4; ++ww) {
            const float4 o = red[wid][ww * 64 + lane];
            s.x += o.x; s.y += o.y; s.z += o.z; s.w += o.w;
        }
        float* dst = (wid == 0 ? a.axp0 : a.axp1) + (size_t)seg * a.ldo + row;
        *reinterpret_cast<float4*>(dst) = s;
    } else {
        float* dst = (wid == 2 ? a.dot0 : a.dot1) + (size_t)rb * a.ldo + t.y;                          // t.y + width <= (rb + 1) * 256 <= ldo
        for (int c = lane * 4; c < t.z; c += 256) *reinterpret_cast<float4*>(dst + c) = *reinterpret_cast<const float4*>(&sdot[wid - 2][c]);
    }
}

// `Extra`: a functor run by ONE additional workgroup (block 0) concurrently with the tiles; the tall
// solver uses it for its scalar iteration control, which then costs no launch and no latency.
struct SymvNoExtra { __device__ void operator()() const {} };

template <typename Extra, bool NT = false, bool MID = false>
__global__ void __launch_bounds__(kSyThreads, 4)      // 4 waves/SIMD: 2 or 4 measure the same, 8 spills; non-temporal loads are 8 % slower (the 2p^2 bytes stay in the Infinity Cache)
symv2_lower_kernel(SymvArgs a, Extra extra) {
    if (blockIdx.x == 0) { extra(); return; }
    // Prologue: the `done` word, this tile's copy of the verdict word and its descriptor are requested together and waited for once --
    // one memory round trip before the first matrix request (round 6 and before: `done`, a branch, then the descriptor: two).
    const int4 t = a.tiles[blockIdx.x - 1];
    const unsigned long long vw = __hip_atomic_load(a.verdict + (size_t)(blockIdx.x & (kSyVerdictReplicas - 1)) * kSyVerdictStride,
                                                    __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int done = *a.skip;
    if (done != 0) return;
    if (vw == a.discard) {                 // this launch's own verdict, already published: nobody reads what this tile would write
        if (threadIdx.x == 0) atomicAdd(a.early, 1ull);
        return;
    }
    __shared__ float4 red[2][kSyThreads];
    __shared__ __attribute__((aligned(16))) float sdot[2][kSyCBMax];
#ifdef ADMM_HIP_PROBE
    const long long pt0 = wall_clock64();
#endif
    symv2_tile<SymvPlainVec, NT, MID>(a, t, SymvPlainVec(), red, sdot);
#ifdef ADMM_HIP_PROBE
    if (a.probe != nullptr && threadIdx.x == 0) {
        const int nt = (int)gridDim.x - 1, t = (int)blockIdx.x - 1;
        const int which = t == 0 ? 0 : (t == nt / 2 ? 1 : (t == nt - 1 ? 2 : (t == (3 * nt) / 4 ? 3 : -1)));
        if (which >= 0) {
            long long* d = a.probe + ((size_t)(a.probe_idx & 4095) * 4 + 3) * 8 + which * 2;
            d[0] = pt0; d[1] = wall_clock64();
        }
    }
#endif
}

// ---- ONE right-hand side, chosen before the stream (the tall solver's default x-update: lasso_tall.hip, SYMV_VERDICT=3).
// symv2_lower_kernel multiplies by both candidates because the decision between them is taken beside its stream.  Everything that decision
// needs was written by EARLIER launches, so every tile can take it itself, in its prologue: a `Gate` functor answers "leave" (nobody
// reads the products of this launch) or which of the two vectors is the one the consumer will read.
//   gate.request()          issues the gate's loads (ordinary cached loads: per XCD one miss per line, the rest L2 hits) and returns them;
//                           called beside the requests of the tile descriptor and the `done` word, so that all arrive in one round trip
//   gate.decide(req, lds)   called by every thread of the workgroup; returns kSyGateLeave, 0 or 1, the same value in every thread
// On "leave" thread 0 counts the tile in `early` and the workgroup returns without writing a partial.  Otherwise the tile is symv2_tile
// for the picked vector alone: per right-hand side the same fmaf chains, the same butterfly8, the same cross-wave sum, the same diagonal
// handling and `last`, so the partials written for pick = r have the bits symv2_lower_kernel writes into plane r -- but they go into
// plane 0 (dot0, axp0) whichever vector was picked, and symv_sum_partials1 below sums that one plane.
// PRE: the first chunk's matrix requests are issued before the gate is evaluated (its block sum and barriers then run under loads in
// flight); that chunk is peeled off the column loop, which keeps the shape that streams best (symv2_tile).
constexpr int kSyGateLeave = -1;
// Every tile of a discarded launch counts itself.  1600 atomic adds to ONE word are served one after the other by the memory side (they
// took 25 us of such a launch, measured; the two-vector kernel's few late leavers never showed it): the tiles spread over kSyEarlySlots
// counters on lines of their own, which the host adds up.
constexpr int kSyEarlySlots = kSyVerdictReplicas;          // a power of two; stride kSyVerdictStride words
constexpr int kSyGateScratch = 6 * (kSyThreads / 64);     // doubles of LDS a gate may use in decide()
struct SymvForcedGate {                                   // a fixed answer (test hook admm_hip_test_symv_one)
    struct Req {};
    int answer;
    __device__ __forceinline__ void pin() const {}        // (a gate's kernel arguments, held in front of the prologue's batch: symv1_tile)
    __device__ __forceinline__ Req request() const { return Req(); }
    __device__ __forceinline__ int decide(const Req&, double*) const { return answer; }
};
#ifndef ADMM_HIP_SYMV1_WGS
#define ADMM_HIP_SYMV1_WGS 4                              // workgroups per CU the one-vector kernel is built for (dev builds: 5, 6; "Measured and rejected" above)
#endif
#ifndef ADMM_HIP_SYMV1_DEPTH
#define ADMM_HIP_SYMV1_DEPTH 2                            // chunks a wave of the packed kernel keeps in flight (dev builds: 1 = request, wait, decode; profiles/tall_two_chunks.md)
#endif
#ifndef ADMM_HIP_SYMV1_PRE
#define ADMM_HIP_SYMV1_PRE 8                              // columns of the first chunk requested ahead of the gate (dev builds: 0 = the gate first; "Measured and rejected" above)
#endif

// Where a tile's 8-column chunk comes from.  symv1_tile below asks a source for (part of) chunk q -- request<K0, K1>(q) issues the loads of
// its columns K0 .. K1 - 1 -- and takes the chunk over as eight float4 (get); everything from there on is one copy of code.
struct SymvTileGeom { int row, col0, last, lane, wid, nqw; };      // nqw: chunks per wave

// The fp32 matrix itself: one float4 per column, columns beyond `last` not loaded (zero).
struct SymvDenseSrc {
    static constexpr int kDepth = 1;      // chunks a wave keeps in flight (117 VGPRs at one: no room for a second)
    static constexpr bool kStraightLine = false;      // every column's load stands under a per-lane branch
    static __device__ __forceinline__ int wave_id() { return threadIdx.x >> 6; }
    struct Desc {};
    __device__ __forceinline__ Desc describe(int) const { return Desc(); }
    __device__ __forceinline__ void pin() const {}      // kernel arguments of its own to hold in the prologue's batch: none
    template <bool NT>
    struct Chunk {
        const float* base; long long lda; int col0, last;
        float4 av[8];
        __device__ __forceinline__ Chunk(const SymvDenseSrc&, const Desc&, const SymvArgs& a, const SymvTileGeom& g)
            : base(a.A + (size_t)g.col0 * a.lda + g.row), lda(a.lda), col0(g.col0), last(g.last) {}
        template <int K0, int K1>
        __device__ __forceinline__ void request(int q) {
#pragma unroll
            for (int k = K0; k < K1; ++k) {
                const int col = col0 + q * 8 + k;
                av[k] = make_float4(0.f, 0.f, 0.f, 0.f);
                if constexpr (NT) { if (col <= last) av[k] = load16_nt<float4>(base + (size_t)(q * 8 + k) * lda); }
                else { if (col <= last) av[k] = *reinterpret_cast<const float4*>(base + (size_t)(q * 8 + k) * lda); }
            }
        }
        template <int B = 0>
        __device__ __forceinline__ void get(int, float4 (&out)[8]) const {
#pragma unroll
            for (int k = 0; k < 8; ++k) out[k] = av[k];
        }
    };
};

// The exact 29-bit copy of the tiles (symv_pack.h; written by symv_pack_kernel below): eight requests per chunk as well, seven of 16 bytes
// and one of 4, all of them issued with the chunk's first column.  A lane whose chunk lies wholly above the diagonal, beyond column p - 1
// or beyond the last row requests nothing and gets zeros (d = 14 everywhere), as the fp32 source's `last` does column by column.
// The requests are buffer loads through a descriptor of the wave's own chunks, and such a lane's offset lies beyond the descriptor's
// range: the range check drops its part of the request and hands back zeros, so the eight loads of a chunk stand in straight-line code.
// (Under a per-lane branch the compiler's wait counts have to cover the path that skipped the loads as well, and the decode of one
// chunk then waits for the chunk requested behind it.)  get() puts the sixteen d = 14 in.
struct SymvPackedSrc {
    const unsigned* stream;      // chunk c of the plan at stream + c * kSpChunkDwords
    const int4* ptile;           // per tile: first chunk, base, escapes listed, escapes met
    const uint2* esc;            // per tile esc_cap entries: (chunk of the tile << 11 | lane << 5 | entry, the float's bits)
    int esc_cap;
    using Desc = int4;
    __device__ __forceinline__ Desc describe(int tile) const { return ptile[tile]; }
    __device__ __forceinline__ void pin() const { asm volatile("" :: "s"(stream), "s"(ptile), "s"(esc), "s"(esc_cap)); }
    static constexpr int kDepth = ADMM_HIP_SYMV1_DEPTH;       // chunks a wave keeps in flight: 2 x 29 of the 128 VGPRs of 4 waves per SIMD
    static constexpr bool kStraightLine = true;               // request(q, exists): dead lanes and missing chunks by offset, no branch
    // the wave's number as a scalar: its first column, its chunk count and its place in the tile's row of dot partials then are scalars too
    static __device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }
    static constexpr unsigned kNoRequest = 0x7FFF0000u;       // a byte offset beyond any wave's chunks (8 x 7424 bytes), immediates added
    struct Rec { uint4 pc[kSpPieces]; unsigned signs; };      // one lane's record of a chunk as it is loaded
    template <bool NT>
    struct Chunk {
        __amdgpu_buffer_rsrc_t chunks;      // the wave's chunks (wave-uniform: built from scalars)
        unsigned off16, off4;               // this lane's byte offsets into the 16-byte pieces and into the sign words of a chunk
        const uint2* esc; int nesc, ebase, col0, last, lane, chunk0;
        Rec ping, pong;                     // two named buffers: while one is decoded the other's loads are in flight (symv1_tile's column loop)
        __device__ __forceinline__ Chunk(const SymvPackedSrc& s, const Desc& d, const SymvArgs&, const SymvTileGeom& g)
            : off16(g.lane * 16u), off4((4u * kSpPieces * 64u + g.lane) * 4u), esc(s.esc + (size_t)(blockIdx.x - 1) * s.esc_cap),
              nesc(d.z), ebase(d.y), col0(g.col0), last(g.last), lane(g.lane), chunk0(g.wid * g.nqw) {
            const int w = g.wid, first = __builtin_amdgcn_readfirstlane(d.x), nqw = __builtin_amdgcn_readfirstlane(g.nqw);
            const unsigned* base = s.stream + ((size_t)first + (size_t)(w * nqw)) * kSpChunkDwords;
            chunks = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned*>(base), 0, nqw * kSpChunkBytes, 0x00020000);
        }
        template <int B> __device__ __forceinline__ Rec& rec() { if constexpr (B == 0) return ping; else return pong; }
        template <int B> __device__ __forceinline__ const Rec& rec() const { if constexpr (B == 0) return ping; else return pong; }
        __device__ __forceinline__ bool requested(int q) const { return col0 + q * 8 <= last; }
        template <int K0, int K1, int B = 0>
        __device__ __forceinline__ void request(int q, bool exists = true) {      // exists: q < the wave's chunks (ahead of the last one there is none)
            if constexpr (K0 == 0 && K1 > 0) {
                typedef unsigned int u4_t __attribute__((ext_vector_type(4)));
                constexpr int aux = NT ? 2 : 0;               // the non-temporal hint of load16_nt
                Rec& r = rec<B>();
                const bool on = exists && requested(q);
                const unsigned at = (unsigned)q * (unsigned)kSpChunkBytes;
                const unsigned o16 = on ? at + off16 : kNoRequest, o4 = on ? at + off4 : kNoRequest;
#pragma unroll
                for (int i = 0; i < kSpPieces; ++i) {
                    const u4_t v = __builtin_amdgcn_raw_buffer_load_b128(chunks, o16 + 1024u * i, 0, aux);
                    r.pc[i] = make_uint4(v.x, v.y, v.z, v.w);
                }
                r.signs = __builtin_amdgcn_raw_buffer_load_b32(chunks, o4, 0, aux);
            }
        }
        template <int B = 0>
        __device__ __forceinline__ void get(int q, float4 (&out)[8]) const {
            const Rec& r = rec<B>();
            unsigned rec[kSpRecDwords], bits[kSpEntries];
#pragma unroll
            for (int i = 0; i < kSpPieces; ++i) { rec[4 * i] = r.pc[i].x; rec[4 * i + 1] = r.pc[i].y; rec[4 * i + 2] = r.pc[i].z; rec[4 * i + 3] = r.pc[i].w; }
            rec[4 * kSpPieces] = r.signs;
            if (!requested(q)) { rec[0] = 0xEEEEEEEEu; rec[1] = 0xEEEEEEEEu; rec[2] = 0xEEEEEEEEu; rec[3] = 0xEEEEEEEEu; }      // d = 14: every entry a zero
#if ADMM_HIP_SYMV_PACK_DEC == 2      // dev build, timing only: the 29 dwords as they come (meaningless products) -- what the stream costs without any decode
#pragma unroll
            for (int e = 0; e < kSpEntries; ++e) bits[e] = rec[e < kSpRecDwords ? e : e - 4] ^ (unsigned)ebase;
#else
            sp_record_decode(rec, ebase, bits);
#endif
#pragma unroll
            for (int k = 0; k < 8; ++k)
                out[k] = make_float4(__uint_as_float(bits[4 * k]), __uint_as_float(bits[4 * k + 1]), __uint_as_float(bits[4 * k + 2]), __uint_as_float(bits[4 * k + 3]));
            if (nesc > 0) {            // wave-uniform, a handful of tiles per launch: the listed floats replace the +0.0 of their places
                const unsigned me = ((unsigned)(chunk0 + q) << 6) | (unsigned)lane;
                for (int i = 0; i < nesc; ++i) {
                    const uint2 en = esc[i];
                    const bool hit = (en.x >> 5) == me;
                    const unsigned e = en.x & 31u;
                    const float val = __uint_as_float(en.y);
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        if (hit && e == 4u * k + 0u) out[k].x = val;
                        if (hit && e == 4u * k + 1u) out[k].y = val;
                        if (hit && e == 4u * k + 2u) out[k].z = val;
                        if (hit && e == 4u * k + 3u) out[k].w = val;
                    }
                }
            }
        }
    };
};

// One tile of the one-vector product, behind the `extra` workgroup's exit: prologue, gate, peeled first chunk, column loop, epilogue.
template <typename Src, typename Gate, bool NT, int PRE>
__device__ __forceinline__ void symv1_tile(const SymvArgs& a, const Src& src, const Gate& gate, float4* red, float* sdot, double* gate_lds) {
    // Prologue: the tile descriptor(s), the `done` word and the gate's inputs are requested together -- everything that needs only
    // blockIdx, threadIdx and kernel arguments leaves in ONE batch, behind the wait for the kernel arguments and ahead of any other wait.
    // Round 11: held there by a compiler-level memory fence in front of the `done` branch (no instruction; without it the descriptor
    // loads and the gate's control block were sunk below the branch, one scalar round trip each) and by gates that do not use what they
    // request before decide() (tests/test_tall_prologue_asm.py reads the compiled order).  The kernel arguments come in one fetch in
    // front of the batch: every one the tile uses is pinned in this block, and the scheduling barrier keeps their fetches, which stand at
    // its head, above the batch (fetched as they were first used, the pointers the batch starts from and the rest came in two or three
    // scalar round trips).  The pins stand BEHIND the batch's loads: an asm statement in front of them makes the compiler read the
    // control words through the vector path.
    __builtin_amdgcn_sched_barrier(0);
    const int4 t = a.tiles[blockIdx.x - 1];
    const int done = *a.skip;
    const typename Gate::Req greq = gate.request();
    const typename Src::Desc sd = src.describe(blockIdx.x - 1);
    asm volatile("" ::: "memory");
    asm volatile("" :: "s"(a.A), "s"(a.lda), "s"(a.p), "s"(a.v0), "s"(a.v1), "s"(a.dot0), "s"(a.axp0), "s"(a.ldo), "s"(a.early));
    src.pin();
    gate.pin();
    __builtin_amdgcn_sched_barrier(0);
    if (done != 0) return;                // (arrives with the descriptor: checked before the first matrix request, not behind it)
    const int rb = t.x, seg = t.w;
    const int cw = t.z >> 2;               // columns per wave: a multiple of 8, at most 64
    const int lane = threadIdx.x & 63, wid = Src::wave_id();
    const int row = rb * kSyRB + lane * 4;
    const int col0 = t.y + wid * cw;
    const int p4 = (a.p + 3) & ~3;
    const bool active = row < p4;
    const bool has = col0 < a.p;           // every wave of a listed tile has all its columns <= the block's last row
    const bool diag = col0 + (cw - 1) >= rb * kSyRB;         // this wave's block meets the diagonal
    const int nq = has ? cw >> 3 : 0;
    const int last = active ? min(a.p - 1, diag ? row + 3 : INT_MAX) : -1;      // symv2_tile's `last`
    const SymvTileGeom geom = {row, col0, last, lane, wid, cw >> 3};
    typename Src::template Chunk<NT> ch(src, sd, a, geom);
    static_assert(PRE >= 0 && PRE <= 8, "columns of the first chunk requested ahead of the gate");
    if constexpr (PRE > 0) {
        // a source whose requests are straight-line code asks without a branch (a wave without columns asks for nothing): behind a
        // branch, the gate's wait for its own loads has to cover the path that skipped the chunk's, and takes part of the chunk in
        if constexpr (Src::kStraightLine) ch.template request<0, PRE>(0, nq > 0);
        else if (nq > 0) ch.template request<0, PRE>(0);
    }
    __builtin_amdgcn_sched_barrier(0);     // the gate's first use of its requests stays behind the chunk's
    const int g = gate.decide(greq, gate_lds);
    if (g == kSyGateLeave) {               // nobody reads what this launch would write: the slots keep what the last consumed launch left
        if (threadIdx.x == 0) atomicAdd(a.early + (size_t)(blockIdx.x & (kSyEarlySlots - 1)) * kSyVerdictStride, 1ull);
        return;
    }
#ifdef ADMM_HIP_PROBE
    const long long pt0 = wall_clock64();
#endif
    const float* v = g != 0 ? a.v1 : a.v0;
    float4 aU = make_float4(0.f, 0.f, 0.f, 0.f);
    if (has) {
        const float4 uI = active ? *reinterpret_cast<const float4*>(v + row) : make_float4(0.f, 0.f, 0.f, 0.f);
        const int cj = col0 + lane;                                          // the wave's (<= 64) right-hand entries, one per lane
        const float uj = (lane < cw && cj < a.p) ? v[cj] : 0.f;
        const auto consume = [&](int q, auto buf) {
            float4 av[8];
            ch.template get<decltype(buf)::value>(q, av);
            float dU[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int col = col0 + q * 8 + k;
                float4 m = av[k];
                float4 ax = m;                                    // axpy part excludes the diagonal
                if (diag) {
                    if (row + 0 < col) m.x = 0.f;
                    if (row + 1 < col) m.y = 0.f;
                    if (row + 2 < col) m.z = 0.f;
                    if (row + 3 < col) m.w = 0.f;
                    ax = m;
                    if (row + 0 == col) ax.x = 0.f;
                    if (row + 1 == col) ax.y = 0.f;
                    if (row + 2 == col) ax.z = 0.f;
                    if (row + 3 == col) ax.w = 0.f;
                }
                dU[k] = fmaf(m.x, uI.x, fmaf(m.y, uI.y, fmaf(m.z, uI.z, m.w * uI.w)));
                const float ujc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(uj), (q * 8 + k) & 63));
                aU.x = fmaf(ax.x, ujc, aU.x); aU.y = fmaf(ax.y, ujc, aU.y); aU.z = fmaf(ax.z, ujc, aU.z); aU.w = fmaf(ax.w, ujc, aU.w);
            }
            const float du = butterfly8(dU, lane);                // every lane ends with column (lane >> 3)
            if ((lane & 7) == 0) sdot[wid * cw + q * 8 + (lane >> 3)] = du;
        };
        constexpr std::integral_constant<int, 0> ping;
        constexpr std::integral_constant<int, 1> pong;
        if constexpr (Src::kDepth == 2) {
            // Two chunks in flight per wave: chunk q + 1 is requested into the other buffer before chunk q is decoded, so a wave is never
            // without an outstanding request while it has columns left.  Unrolled by two by hand over the two named buffers -- no register
            // moves between them; the request ahead of a wave's last chunk asks for nothing.
            if constexpr (PRE > 0) ch.template request<PRE, 8, 0>(0); else ch.template request<0, 8, 0>(0);
#pragma unroll 1
            for (int q = 0; q < nq; q += 2) {             // chunk q is in ping
                __builtin_amdgcn_sched_barrier(0);
                ch.template request<0, 8, 1>(q + 1, q + 1 < nq);
                __builtin_amdgcn_sched_barrier(0);
                consume(q, ping);
                if (q + 1 >= nq) break;
                __builtin_amdgcn_sched_barrier(0);
                ch.template request<0, 8, 0>(q + 2, q + 2 < nq);
                __builtin_amdgcn_sched_barrier(0);
                consume(q + 1, pong);
            }
        } else {
            if constexpr (PRE > 0) { ch.template request<PRE, 8>(0); consume(0, ping); }      // the rest of the peeled chunk
#pragma unroll 1
            for (int q = PRE > 0 ? 1 : 0; q < nq; ++q) {
                ch.template request<0, 8>(q);
                consume(q, ping);
            }
        }
    } else {
        for (int c = lane; c < cw; c += 64) sdot[wid * cw + c] = 0.f;
    }
    // axpy part: wave 0 adds the 4 waves (same rows, different columns) in symv2_tile's order; dot part: wave 1 writes the one row
    red[threadIdx.x] = aU;
    __syncthreads();
    if (wid == 0) {
        float4 s = red[lane];
#pragma unroll
        for (int ww = 1; ww < 4; ++ww) {
            const float4 o = red[ww * 64 + lane];
            s.x += o.x; s.y += o.y; s.z += o.z; s.w += o.w;
        }
        *reinterpret_cast<float4*>(a.axp0 + (size_t)seg * a.ldo + row) = s;
    } else if (wid == 1) {
        float* dst = a.dot0 + (size_t)rb * a.ldo + t.y;                          // t.y + width <= (rb + 1) * 256 <= ldo
        for (int c = lane * 4; c < t.z; c += 256) *reinterpret_cast<float4*>(dst + c) = *reinterpret_cast<const float4*>(&sdot[c]);
    }
#ifdef ADMM_HIP_PROBE
    if (a.probe != nullptr && threadIdx.x == 0) {
        const int nt = (int)gridDim.x - 1, ti = (int)blockIdx.x - 1;
        const int which = ti == 0 ? 0 : (ti == nt / 2 ? 1 : (ti == nt - 1 ? 2 : (ti == (3 * nt) / 4 ? 3 : -1)));
        if (which >= 0) {
            long long* d = a.probe + ((size_t)(a.probe_idx & 4095) * 4 + 3) * 8 + which * 2;
            d[0] = pt0; d[1] = wall_clock64();
        }
    }
#endif
}

template <typename Gate, typename Extra, bool NT = false, int PRE = ADMM_HIP_SYMV1_PRE>
__global__ void __launch_bounds__(kSyThreads, ADMM_HIP_SYMV1_WGS)
symv1_lower_kernel(SymvArgs a, Gate gate, Extra extra) {
    if (blockIdx.x == 0) { extra(); return; }
    __shared__ float4 red[kSyThreads];
    __shared__ __attribute__((aligned(16))) float sdot[kSyCBMax];
    __shared__ double gate_lds[kSyGateScratch];
    symv1_tile<SymvDenseSrc, Gate, NT, PRE>(a, SymvDenseSrc(), gate, red, sdot, gate_lds);
}

// The same kernel on the 29-bit copy of the tiles: 181.25 instead of 200 bytes per 50 entries, decoded to the bits of the fp32 matrix.
template <typename Gate, typename Extra, bool NT = false, int PRE = ADMM_HIP_SYMV1_PRE>
__global__ void __launch_bounds__(kSyThreads, ADMM_HIP_SYMV1_WGS)
symv1_packed_kernel(SymvArgs a, SymvPackedSrc src, Gate gate, Extra extra) {
    if (blockIdx.x == 0) { extra(); return; }
    __shared__ float4 red[kSyThreads];
    __shared__ __attribute__((aligned(16))) float sdot[kSyCBMax];
    __shared__ double gate_lds[kSyGateScratch];
    symv1_tile<SymvPackedSrc, Gate, NT, PRE>(a, src, gate, red, sdot, gate_lds);
}

// Packs the tiles of a plan: one workgroup per tile, thread = (wave, lane) of the streaming kernel.  First the tile's base (the largest
// upper-seven-bit exponent among the entries the fp32 kernel uses that are finite and not zero), then record by record.  Entries the fp32
// kernel never uses -- above the diagonal, rows >= p rounded up to 4, columns >= p -- are +0.0 and are not read from the matrix.
struct SymvPackArgs {
    const float* A; long long lda; int p;
    const int4* tiles;
    int4* ptile;                       // x (first chunk) is given; y, z, w are written: base, escapes listed, escapes met
    unsigned* stream;
    uint2* esc; int esc_cap;
    unsigned long long* totals;        // [0] escapes met, [1] tiles whose list overflowed
};
static __global__ void __launch_bounds__(kSyThreads)
symv_pack_kernel(SymvPackArgs a) {
    __shared__ int s_base;
    __shared__ unsigned s_cnt;
    const int4 t = a.tiles[blockIdx.x];
    const int rb = t.x, cw = t.z >> 2, nqw = cw >> 3;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int row = rb * kSyRB + lane * 4;
    const int col0 = t.y + wid * cw;
    const int p4 = (a.p + 3) & ~3;
    const bool active = row < p4;
    if (threadIdx.x == 0) { s_base = 0; s_cnt = 0u; }
    __syncthreads();
    const float* base = a.A + (size_t)col0 * a.lda + row;
    const auto column = [&](int j, unsigned (&b)[4]) {      // the four entries of this lane in column col0 + j, unused ones as +0.0
        const int col = col0 + j;
        b[0] = b[1] = b[2] = b[3] = 0u;
        if (active && col < a.p && row + 3 >= col) {
            const float4 m = *reinterpret_cast<const float4*>(base + (size_t)j * a.lda);
            if (row + 0 >= col) b[0] = __float_as_uint(m.x);
            if (row + 1 >= col) b[1] = __float_as_uint(m.y);
            if (row + 2 >= col) b[2] = __float_as_uint(m.z);
            b[3] = __float_as_uint(m.w);
        }
    };
    int mx = 0;
    for (int j = 0; j < cw; ++j) {
        unsigned b[4];
        column(j, b);
#pragma unroll
        for (int c = 0; c < 4; ++c) if (sp_counts(b[c])) mx = max(mx, sp_exp7(b[c]));
    }
    atomicMax(&s_base, mx);
    __syncthreads();
    const int ebase = s_base;
    const size_t first = (size_t)a.ptile[blockIdx.x].x;
    for (int q = 0; q < nqw; ++q) {
        unsigned bits[kSpEntries], rec[kSpRecDwords];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            unsigned b[4];
            column(q * 8 + k, b);
            bits[4 * k] = b[0]; bits[4 * k + 1] = b[1]; bits[4 * k + 2] = b[2]; bits[4 * k + 3] = b[3];
        }
        const unsigned em = sp_record_encode(bits, ebase, rec);
        unsigned* c = a.stream + (first + (size_t)(wid * nqw + q)) * kSpChunkDwords;
#pragma unroll
        for (int i = 0; i < kSpPieces; ++i)
            *reinterpret_cast<uint4*>(c + (i * 64 + lane) * 4) = make_uint4(rec[4 * i], rec[4 * i + 1], rec[4 * i + 2], rec[4 * i + 3]);
        c[4 * kSpPieces * 64 + lane] = rec[4 * kSpPieces];
        if (em != 0u) {
#pragma unroll
            for (int e = 0; e < kSpEntries; ++e) {
                if ((em >> e) & 1u) {
                    const unsigned slot = atomicAdd(&s_cnt, 1u);
                    if (slot < (unsigned)a.esc_cap)
                        a.esc[(size_t)blockIdx.x * a.esc_cap + slot] = make_uint2(((unsigned)(wid * nqw + q) << 11) | ((unsigned)lane << 5) | (unsigned)e, bits[e]);
                }
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned n = s_cnt;
        int4 d = a.ptile[blockIdx.x];
        d.y = ebase; d.z = (int)min(n, (unsigned)a.esc_cap); d.w = (int)n;
        a.ptile[blockIdx.x] = d;
        if (n != 0u) atomicAdd(a.totals, (unsigned long long)n);
        if (n > (unsigned)a.esc_cap) atomicAdd(a.totals + 1, 1ull);
    }
}

// ---- NR right-hand sides on ONE load of every matrix element (multi-task lasso: lasso_tall.hip, tall_mt_tail_kernel).
// symv2_lower_kernel streams 2 p^2 bytes for two vectors; with one cached inverse shared by m responses the same bytes can serve
// all 2 m of them.  Same tile list (SymvPlan, SymvSched), same partial layout, one PLANE of partials per right-hand side.  For every
// right-hand side the arithmetic is symv2_tile's to the bit -- the same fmaf chains, the same butterfly8, the same cross-wave sum of
// the axpy part -- so a partial does not depend on which other vectors share the pass: NR is invisible in the results, and
// NR = 2 reproduces symv2_lower_kernel.
// Registers: 4 NR (row entries) + NR (column entries) + 4 NR (axpy accumulators) + 32 (the 8-column chunk); waves that meet the
// diagonal hold a second, diagonal-free copy of the chunk, the others do not (two copies of the chunk body).  2 waves per SIMD
// (at 4 every NR spills); the cross-wave sums go pair by pair through the one [2][256] float4 buffer, LDS = 8 KB + NR KB.
struct SymvNArgs {
    const float* A; long long lda; int p;
    const float* v; long long vstride;     // right-hand vector r of this pass: v + r * vstride (allocated and zero padded to a multiple of 256)
    float* dot; long long dot_stride;      // its planes of partials: dot + r * dot_stride is [nrb][ldo], axp + r * axp_stride is [nax_rows][ldo]
    float* axp; long long axp_stride;
    int nvec;                              // vectors of this pass, 1 .. NR (the kernel computes NR: slots beyond nvec repeat the last vector and store nothing)
    long long ldo;
    const int4* tiles;
    const int* skip;
};
constexpr int kSyNR[] = {2, 4, 8, 12};    // the instantiations built (MT_RHS, options.h); every one compiles without scratch
constexpr int kSyNRCount = (int)(sizeof(kSyNR) / sizeof(kSyNR[0]));

// the 8-column chunk against the NR vectors.  DIAG: the wave's block meets the diagonal (upper entries dropped, the axpy part without the diagonal)
template <int NR, bool DIAG>
__device__ __forceinline__ void symvn_chunk(float4 (&av)[8], const float4 (&vI)[NR], const float (&vj)[NR], float4 (&acc)[NR],
                                            int row, int colq, int q, int lane, float (*sdot)[kSyCBMax], int sbase) {
    float4 ax[DIAG ? 8 : 1];
    if (DIAG) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int col = colq + k;
            float4 v = av[k];
            if (row + 0 < col) v.x = 0.f;
            if (row + 1 < col) v.y = 0.f;
            if (row + 2 < col) v.z = 0.f;
            if (row + 3 < col) v.w = 0.f;
            av[k] = v;
            if (row + 0 == col) v.x = 0.f;
            if (row + 1 == col) v.y = 0.f;
            if (row + 2 == col) v.z = 0.f;
            if (row + 3 == col) v.w = 0.f;
            ax[DIAG ? k : 0] = v;
        }
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        float d[8];
        const float4 xi = vI[r];
        float4 s = acc[r];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float4 v = av[k];
            const float4 x = DIAG ? ax[DIAG ? k : 0] : av[k];
            d[k] = fmaf(v.x, xi.x, fmaf(v.y, xi.y, fmaf(v.z, xi.z, v.w * xi.w)));
            const float c = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(vj[r]), (q * 8 + k) & 63));
            s.x = fmaf(x.x, c, s.x); s.y = fmaf(x.y, c, s.y); s.z = fmaf(x.z, c, s.z); s.w = fmaf(x.w, c, s.w);
        }
        acc[r] = s;
        const float dr = butterfly8(d, lane);
        if ((lane & 7) == 0) sdot[r][sbase + (lane >> 3)] = dr;
    }
}

template <int NR, typename Extra, bool NT = false>
__global__ void __launch_bounds__(kSyThreads, 2)
symvn_lower_kernel(SymvNArgs a, Extra extra) {
    static_assert(NR >= 2 && NR % 2 == 0, "right-hand sides come in pairs (u_k, w_k)");
    if (blockIdx.x == 0) { extra(); return; }
    if (a.skip != nullptr && *a.skip != 0) return;
    __shared__ float4 red[2][kSyThreads];
    __shared__ __attribute__((aligned(16))) float sdot[NR][kSyCBMax];
    const int4 t = a.tiles[blockIdx.x - 1];
    const int rb = t.x, seg = t.w;
    const int cw = t.z >> 2;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int row = rb * kSyRB + lane * 4;
    const int col0 = t.y + wid * cw;
    const int p4 = (a.p + 3) & ~3;
    const bool active = row < p4;
    const bool has = col0 < a.p;
    const float* base = a.A + (size_t)col0 * a.lda + row;
    float4 acc[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = make_float4(0.f, 0.f, 0.f, 0.f);

    if (has) {
        float4 vI[NR];
        float vj[NR];
        const int cj = col0 + lane;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const float* vr = a.v + (size_t)min(r, a.nvec - 1) * a.vstride;
            vI[r] = active ? *reinterpret_cast<const float4*>(vr + row) : make_float4(0.f, 0.f, 0.f, 0.f);
            vj[r] = (lane < cw && cj < a.p) ? vr[cj] : 0.f;
        }
        const bool diag = col0 + (cw - 1) >= rb * kSyRB;
        const int nq = cw >> 3;
#pragma unroll 1
        for (int q = 0; q < nq; ++q) {
            float4 av[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int col = col0 + q * 8 + k;
                av[k] = make_float4(0.f, 0.f, 0.f, 0.f);
                if constexpr (NT) { if (active && col < a.p) av[k] = load16_nt<float4>(base + (size_t)(q * 8 + k) * a.lda); }
                else { if (active && col < a.p) av[k] = *reinterpret_cast<const float4*>(base + (size_t)(q * 8 + k) * a.lda); }
            }
            if (diag) symvn_chunk<NR, true>(av, vI, vj, acc, row, col0 + q * 8, q, lane, sdot, wid * cw + q * 8);
            else symvn_chunk<NR, false>(av, vI, vj, acc, row, col0 + q * 8, q, lane, sdot, wid * cw + q * 8);
        }
    } else {
#pragma unroll
        for (int r = 0; r < NR; ++r)
            for (int c = lane; c < cw; c += 64) sdot[r][wid * cw + c] = 0.f;
    }
    // pair by pair, as symv2_tile does for its one pair: waves 0 / 1 add the 4 waves' axpy parts of vectors 2 pr / 2 pr + 1, waves 2 / 3 write their dot rows
#pragma unroll
    for (int pr = 0; pr < NR / 2; ++pr) {
        if (pr > 0) __syncthreads();
        red[0][threadIdx.x] = acc[2 * pr];
        red[1][threadIdx.x] = acc[2 * pr + 1];
        __syncthreads();
        const int r = 2 * pr + (wid & 1);
        if (r >= a.nvec) continue;
        if (wid < 2) {
            float4 s = red[wid][lane];
#pragma unroll
            for (int ww = 1; ww < 4; ++ww) {
                const float4 o = red[wid][ww * 64 + lane];
                s.x += o.x; s.y += o.y; s.z += o.z; s.w += o.w;
            }
            float* dst = a.axp + (size_t)r * a.axp_stride + (size_t)seg * a.ldo + row;
            *reinterpret_cast<float4*>(dst) = s;
        } else {
            float* dst = a.dot + (size_t)r * a.dot_stride + (size_t)rb * a.ldo + t.y;
            for (int c = lane * 4; c < t.z; c += 256) *reinterpret_cast<float4*>(dst + c) = *reinterpret_cast<const float4*>(&sdot[r][c]);
        }
    }
}

// Mixed-precision refinement of the tall x-update (opt-in, ADMM_HIP_REFINE=1; lasso_tall.hip): the products M x0, M x1 of the
// float system matrix M = X'X + rho I (lower triangle read, both halves of the symmetric product per loaded element, as
// above) with the two float vectors x0, x1, every product and every sum in DOUBLE -- the residual of a refinement step has
// to be formed more accurately than the solve it corrects.  Same tiles, same partial layout, double partial arrays.  Not
// tuned like the float kernel (a refined iteration streams the triangle three times anyway).
struct SymvArgsD {
    const float* A; long long lda; int p;
    const float* v0; const float* v1;
    double* dot0; double* dot1; double* axp0; double* axp1;
    long long ldo;
    const int4* tiles;
    const int* skip;
};
static __global__ void __launch_bounds__(kSyThreads, 2)
symv2_lower_f64acc_kernel(SymvArgsD a) {
    if (a.skip != nullptr && *a.skip != 0) return;
    __shared__ double4 red[2][kSyThreads];
    __shared__ __attribute__((aligned(16))) double sdot[2][kSyCBMax];
    const int4 t = a.tiles[blockIdx.x];
    const int rb = t.x, seg = t.w, cw = t.z >> 2;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int row = rb * kSyRB + lane * 4;
    const int col0 = t.y + wid * cw;
    const int p4 = (a.p + 3) & ~3;
    const bool active = row < p4, has = col0 < a.p;
    const float* base = a.A + (size_t)col0 * a.lda + row;
    double4 aU = make_double4(0, 0, 0, 0), aW = aU;
    if (has) {
        const float4 uI = active ? *reinterpret_cast<const float4*>(a.v0 + row) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 wI = active ? *reinterpret_cast<const float4*>(a.v1 + row) : make_float4(0.f, 0.f, 0.f, 0.f);
        const int cj = col0 + lane;
        const float uj = (lane < cw && cj < a.p) ? a.v0[cj] : 0.f;
        const float wj = (lane < cw && cj < a.p) ? a.v1[cj] : 0.f;
        const bool diag = col0 + (cw - 1) >= rb * kSyRB;
        for (int q = 0; q < (cw >> 3); ++q) {
            double dU[8], dW[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int col = col0 + q * 8 + k;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (active && col < a.p) v = *reinterpret_cast<const float4*>(base + (size_t)(q * 8 + k) * a.lda);
                float4 ax = v;
                if (diag) {
                    if (row + 0 < col) v.x = 0.f;
                    if (row + 1 < col) v.y = 0.f;
                    if (row + 2 < col) v.z = 0.f;
                    if (row + 3 < col) v.w = 0.f;
                    ax = v;
                    if (row + 0 == col) ax.x = 0.f;
                    if (row + 1 == col) ax.y = 0.f;
                    if (row + 2 == col) ax.z = 0.f;
                    if (row + 3 == col) ax.w = 0.f;
                }
                dU[k] = (double)v.x * uI.x + (double)v.y * uI.y + (double)v.z * uI.z + (double)v.w * uI.w;
                dW[k] = (double)v.x * wI.x + (double)v.y * wI.y + (double)v.z * wI.z + (double)v.w * wI.w;
                const double ujc = (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(uj), (q * 8 + k) & 63));
                const double wjc = (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(wj), (q * 8 + k) & 63));
                aU.x += ax.x * ujc; aU.y += ax.y * ujc; aU.z += ax.z * ujc; aU.w += ax.w * ujc;
                aW.x += ax.x * wjc; aW.y += ax.y * wjc; aW.z += ax.z * wjc; aW.w += ax.w * wjc;
            }
            const double du = butterfly8(dU, lane), dw = butterfly8(dW, lane);
            if ((lane & 7) == 0) { sdot[0][wid * cw + q * 8 + (lane >> 3)] = du; sdot[1][wid * cw + q * 8 + (lane >> 3)] = dw; }
        }
    } else {
        for (int c = lane; c < cw; c += 64) { sdot[0][wid * cw + c] = 0.0; sdot[1][wid * cw + c] = 0.0; }
    }
    red[0][threadIdx.x] = aU;
    red[1][threadIdx.x] = aW;
    __syncthreads();
    if (wid < 2) {
        double4 s = red[wid][lane];
#pragma unroll
        for (int ww = 1; ww < 4; ++ww) { const double4 o = red[wid][ww * 64 + lane]; s.x += o.x; s.y += o.y; s.z += o.z; s.w += o.w; }
        double* dst = (wid == 0 ? a.axp0 : a.axp1) + (size_t)seg * a.ldo + row;
        dst[0] = s.x; dst[1] = s.y; dst[2] = s.z; dst[3] = s.w;
    } else {
        double* dst = (wid == 2 ? a.dot0 : a.dot1) + (size_t)rb * a.ldo + t.y;
        for (int c = lane; c < t.z; c += 64) dst[c] = sdot[wid - 2][c];
    }
}

// Number of row blocks, the segment schedule and the tile list: everything of a plan that is decided on the host from numbers alone
// (symv_plan_layout below; SymvPlan::init adds the device storage).  Needs no device: the test hook admm_hip_test_symv_plan returns it.
struct SymvLayout {
    int p = 0, nrb = 0, ncb = 0, p32 = 0;
    int nax_rows = 0;              // rows of the axpy partial arrays = the largest number of segments of one strip
    SymvSched sched;
    long long ldo = 0;
    bool nt = false;
    std::vector<int4> tiles;
};

// cus: compute units of the device the plan is for.  part / nparts: only the tiles whose 128-column group (index in the full list)
// % nparts == part -- the row-sharded tall x-update gives every rank an equal share of the triangle; the partial arrays keep the full
// shape (slots of tiles owned by other ranks stay zero) so that the same consumer code sums them.  Reads the calling thread's SYMV_SCHED.
inline SymvLayout symv_plan_layout(int p, int cus, int part, int nparts) {
    SymvLayout L;
    const int p32 = (p + 31) / 32 * 32;
    const int nrb = (p + kSyRB - 1) / kSyRB;
    L.p = p; L.p32 = p32; L.nrb = nrb;
    L.ncb = (p + kSyCB - 1) / kSyCB;
    L.ldo = (long long)nrb * kSyRB;
    SymvSched sched;
    // Segment schedule (measured on one MI355X with scripts/symv_sched_sweep.py, profiles/r03_symv_sched.md; it/s of the
    // whole 100-lambda loop against round 2's fixed 256 x 128 tiles):
    //   * while the triangle is small enough, the narrowest segments that still fit ONE resident round of workgroups
    //     (4 per CU): more workgroups in flight and no second round -- p = 2048 / 3000: 32 columns, +41 % / +32 %;
    //     p = 4096: 64 columns, +14 % (32 columns would need a second round there: -17 %);
    //   * beyond that two classes: wide segments for the long strips, dispatched first, narrow ones (64) for the short
    //     strips at the end of the launch, so that its end is made of small work units -- p = 6000 / 8000: 128 | 64,
    //     +8 % / +7 %; p = 10^4: 192 | 64, +5..7 % (38.8-39.6 instead of 41.7 us per iteration); p = 16000: +8 %.
    // ADMM_HIP_SYMV_SCHED=big,small,split_permille overrides it ("128,128,0" = round 2's tiling).
    auto count = [&](const SymvSched& sc) { long long t = 0; for (int rb = 0; rb < nrb; ++rb) t += sc.nseg(rb, p32); return t; };
    const long long slots = 4ll * cus * std::max(1, nparts);      // a rank of the row-sharded solver launches 1 / nparts of the tiles
    auto uniform = [](int w) { SymvSched sc; sc.width_big = sc.width_small = w; sc.rb_split = 0; return sc; };
    auto two = [&](int wb, int ws) { SymvSched sc; sc.width_big = wb; sc.width_small = ws; sc.rb_split = nrb / 2; return sc; };
    if (4 * count(uniform(32)) <= 3 * slots) sched = uniform(32);
    else if (count(uniform(64)) <= slots) sched = uniform(64);
    else if (10 * count(two(128, 64)) <= 14 * slots) sched = two(128, 64);
    else sched = two(192, 64);
    if (const OptValue* v = opt(Opt::SYMV_SCHED)) {
        sched.width_big = v->sched[0]; sched.width_small = v->sched[1]; sched.rb_split = (int)((long long)v->sched[2] * nrb / 1000);
    }
    std::vector<int4> h;
    int nax_rows = 1;
    // long row strips first so that the end of the launch is made of the short strips' (narrow) segments
    for (int rb = nrb - 1; rb >= 0; --rb) {
        const int w = sched.width(rb), ns = sched.nseg(rb, p32);
        nax_rows = std::max(nax_rows, ns);
        for (int sg = 0; sg < ns; ++sg) {
            const int c0 = sg * w;
            const int cols = std::min((rb + 1) * kSyRB, p32);
            h.push_back(make_int4(rb, c0, std::min(w, cols - c0), sg));
        }
    }
    if (nparts > 1) {
        // Dealt out in groups of segments that cover whole 128-column blocks of one strip (segment widths of 32 / 64 / 128: 128
        // columns; 192: 384), not segment by segment: the distributed factorisation (chol_inverse.h) forms, of the inverse,
        // only the 128 x 128 tiles a rank reads here -- interleaved 32-column segments made every rank read every tile
        // (measured: 0.78 p^3 flops per rank of 2 where 0.59 p^3 is the share).
        auto gcd = [](int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; };
        std::vector<int4> mine;
        int group = -1, last_rb = -1, last_cg = -1;
        for (const int4& t : h) {
            const int w = sched.width(t.x);
            const int gw = w / gcd(w, 128) * 128;
            const int cg = t.y / gw;
            if (t.x != last_rb || cg != last_cg) { ++group; last_rb = t.x; last_cg = cg; }
            if (group % nparts == part) mine.push_back(t);
        }
        h.swap(mine);
    }
    // The whole triangle is re-read every iteration.  Plain loads while most of it stays in the 256 MB Infinity Cache
    // between two passes, non-temporal beyond.  Measured crossover (one MI355X, plain vs nt, TB/s on 2p^2 bytes):
    // p = 10000 5.7 vs 5.3 | 11000 5.90 vs 5.24 | 12000 6.08 vs 5.41 | 13000 4.31 vs 5.50 | 16000 4.1-4.4 vs 5.3-5.4.
    // (a rank of the row-sharded solver re-reads only its 1 / nparts share)
    L.nt = (size_t)2 * (size_t)p * (size_t)p / (size_t)std::max(1, nparts) > (size_t)310000000;
    L.sched = sched; L.nax_rows = nax_rows;
    L.tiles.swap(h);
    return L;
}

// The layout with its device storage: the tile list, the partial arrays (zeroed) and the zero words.
struct SymvPlan {
    int p = 0, nrb = 0, ncb = 0, ntiles = 0, p32 = 0;
    int nax_rows = 0;
    SymvSched sched;
    long long ldo = 0;
    DevBuf<int4> tiles;
    std::vector<int4> htiles;      // host copy of this plan's tile list (the distributed setup derives from it which tiles of the inverse a rank reads)
    bool nt = false;
    DevBuf<float> dot0, dot1, axp0, axp1;
    DevBuf<unsigned long long> zero;      // zeros, the size of the verdict words (the kernel indexes its copy whatever it is given): the `done` word and the verdict of launches that have none
#ifdef ADMM_HIP_PROBE
    long long* probe = nullptr; mutable int probe_idx = 0;
#endif
    void init(int p_, hipStream_t st, int part = 0, int nparts = 1) {
        int cus = 256;
        { int dev = 0; hipDeviceProp_t prop; if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount; }
        SymvLayout L = symv_plan_layout(p_, cus, part, nparts);
        p = L.p; nrb = L.nrb; ncb = L.ncb; p32 = L.p32; nax_rows = L.nax_rows; sched = L.sched; ldo = L.ldo; nt = L.nt;
        htiles.swap(L.tiles);
        const std::vector<int4>& h = htiles;
        ntiles = (int)h.size();
        tiles.alloc(std::max<size_t>(h.size(), 1));
        if (!h.empty()) ADMM_HIP_CHECK(hipMemcpyAsync(tiles.get(), h.data(), h.size() * sizeof(int4), hipMemcpyHostToDevice, st));
        dot0.alloc((size_t)nrb * ldo); dot1.alloc((size_t)nrb * ldo);
        axp0.alloc((size_t)nax_rows * ldo); axp1.alloc((size_t)nax_rows * ldo);
        dot0.zero(st); dot1.zero(st); axp0.zero(st); axp1.zero(st);
        zero.alloc((size_t)kSyVerdictReplicas * kSyVerdictStride); zero.zero(st);
        ADMM_HIP_CHECK(hipStreamSynchronize(st));
    }
    SymvArgs args(const float* A, long long lda, const float* v0, const float* v1, const int* skip, const SymvVerdict& vd = SymvVerdict()) const {
        SymvArgs a;
        a.A = A; a.lda = lda; a.p = p; a.v0 = v0; a.v1 = v1;
        a.dot0 = dot0.get(); a.dot1 = dot1.get(); a.axp0 = axp0.get(); a.axp1 = axp1.get();
        a.ldo = ldo; a.tiles = tiles.get();
        // the kernel loads both words unconditionally (no branch in front of its first requests): without a `done` word or a verdict
        // they are the plan's zero words, which no `discard` value equals (a published word always has its run number set)
        a.skip = skip != nullptr ? skip : reinterpret_cast<const int*>(zero.get());
        a.verdict = vd.words != nullptr ? vd.words : zero.get();
        a.discard = vd.words != nullptr ? vd.discard : ~0ull;
        a.early = vd.early;
#ifdef ADMM_HIP_PROBE
        a.probe = probe; a.probe_idx = probe_idx++;
#endif
        return a;
    }
    template <typename Extra = SymvNoExtra>
    void launch(const float* A, long long lda, const float* v0, const float* v1, const int* skip, hipStream_t st, Extra extra = Extra(),
                hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr, const SymvVerdict& vd = SymvVerdict()) {
        const SymvArgs a = args(A, lda, v0, v1, skip, vd);
        // start/stop events (when given) time exactly this kernel on its stream (hipExtLaunchKernel)
        if (nt) {
            if (ev_start == nullptr && ev_stop == nullptr) hipLaunchKernelGGL((symv2_lower_kernel<Extra, true>), dim3(ntiles + 1), dim3(kSyThreads), 0, st, a, extra);
            else hipExtLaunchKernelGGL((symv2_lower_kernel<Extra, true>), dim3(ntiles + 1), dim3(kSyThreads), 0, st, ev_start, ev_stop, 0, a, extra);
            return;
        }
        if (vd.words != nullptr && vd.mid) {
            if (ev_start == nullptr && ev_stop == nullptr) hipLaunchKernelGGL((symv2_lower_kernel<Extra, false, true>), dim3(ntiles + 1), dim3(kSyThreads), 0, st, a, extra);
            else hipExtLaunchKernelGGL((symv2_lower_kernel<Extra, false, true>), dim3(ntiles + 1), dim3(kSyThreads), 0, st, ev_start, ev_stop, 0, a, extra);
            return;
        }
        if (ev_start == nullptr && ev_stop == nullptr) hipLaunchKernelGGL((symv2_lower_kernel<Extra>), dim3(ntiles + 1), dim3(kSyThreads), 0, st, a, extra);
        else hipExtLaunchKernelGGL((symv2_lower_kernel<Extra>), dim3(ntiles + 1), dim3(kSyThreads), 0, st, ev_start, ev_stop, 0, a, extra);
    }
    // symv1_lower_kernel: the vector `gate` picks (v0 or v1) into plane 0, or nothing at all; `early`: kSyEarlySlots counters (stride
    // kSyVerdictStride words) of the tiles that left, to be added up by the caller
    template <typename Gate, typename Extra = SymvNoExtra>
    void launch_one(const float* A, long long lda, const float* v0, const float* v1, const int* skip, hipStream_t st, Gate gate, unsigned long long* early,
                    Extra extra = Extra(), hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr) {
        SymvVerdict vd;
        vd.early = early;
        const SymvArgs a = args(A, lda, v0, v1, skip, vd);
        const bool timed = ev_start != nullptr || ev_stop != nullptr;
        if (nt) {
            if (!timed) hipLaunchKernelGGL((symv1_lower_kernel<Gate, Extra, true>), dim3(ntiles + 1), dim3(kSyThreads), 0, st, a, gate, extra);
            else hipExtLaunchKernelGGL((symv1_lower_kernel<Gate, Extra, true>), dim3(ntiles + 1), dim3(kSyThreads), 0, st, ev_start, ev_stop, 0, a, gate, extra);
            return;
        }
        if (!timed) hipLaunchKernelGGL((symv1_lower_kernel<Gate, Extra>), dim3(ntiles + 1), dim3(kSyThreads), 0, st, a, gate, extra);
        else hipExtLaunchKernelGGL((symv1_lower_kernel<Gate, Extra>), dim3(ntiles + 1), dim3(kSyThreads), 0, st, ev_start, ev_stop, 0, a, gate, extra);
    }
};

// The 29-bit copy of a plan's tiles (symv_pack.h) with its per-tile descriptors and escape lists.  build() packs once per inverse and
// tile list; a list that overflows its capacity leaves `ready` false and the caller on the fp32 stream.
struct SymvPacked {
    DevBuf<unsigned> stream;
    DevBuf<int4> ptile;
    DevBuf<uint2> esc;
    DevBuf<unsigned long long> totals;
    int esc_cap = kSpEscCap;
    size_t chunks = 0;
    unsigned long long escapes = 0, overflowed = 0;      // escapes met over all tiles; tiles whose list overflowed
    bool ready = false, nt = false;
    size_t bytes() const { return chunks * (size_t)kSpChunkBytes; }
    static size_t bytes_for(const SymvPlan& sy) {      // of the copy of that plan's tiles, before anything is allocated
        size_t c = 0;
        for (const int4& t : sy.htiles) c += (size_t)(t.z >> 3);
        return c * (size_t)kSpChunkBytes;
    }
    void release() { stream.release(); ptile.release(); esc.release(); totals.release(); chunks = 0; ready = false; }
    bool build(const SymvPlan& sy, const float* A, long long lda, hipStream_t st, int cap = kSpEscCap) {
        ready = false;
        esc_cap = cap;
        std::vector<int4> h((size_t)std::max(sy.ntiles, 1), make_int4(0, 0, 0, 0));
        chunks = 0;
        for (int k = 0; k < sy.ntiles; ++k) { h[k].x = (int)chunks; chunks += (size_t)(sy.htiles[k].z >> 3); }
        if (sy.ntiles == 0) return false;
        stream.alloc(chunks * (size_t)kSpChunkDwords);
        ptile.alloc(h.size());
        esc.alloc(std::max<size_t>((size_t)sy.ntiles * (size_t)cap, 1));
        totals.alloc(2); totals.zero(st);
        ADMM_HIP_CHECK(hipMemcpyAsync(ptile.get(), h.data(), h.size() * sizeof(int4), hipMemcpyHostToDevice, st));
        SymvPackArgs a;
        a.A = A; a.lda = lda; a.p = sy.p; a.tiles = sy.tiles.get(); a.ptile = ptile.get(); a.stream = stream.get();
        a.esc = esc.get(); a.esc_cap = cap; a.totals = totals.get();
        hipLaunchKernelGGL(symv_pack_kernel, dim3(sy.ntiles), dim3(kSyThreads), 0, st, a);
        ADMM_HIP_CHECK(hipGetLastError());
        unsigned long long tt[2] = {0, 0};
        ADMM_HIP_CHECK(hipMemcpyAsync(tt, totals.get(), sizeof(tt), hipMemcpyDeviceToHost, st));
        ADMM_HIP_CHECK(hipStreamSynchronize(st));      // (also keeps `h` alive until it is copied)
        escapes = tt[0]; overflowed = tt[1];
        nt = bytes() > (size_t)310000000;              // the fp32 stream's crossover (symv_plan_layout) on the bytes streamed here
        ready = overflowed == 0;
        return ready;
    }
    SymvPackedSrc src() const { return SymvPackedSrc{stream.get(), ptile.get(), esc.get(), esc_cap}; }
};

// SymvPlan::launch_one on the packed copy: same gate, same partials into plane 0.
template <typename Gate, typename Extra = SymvNoExtra>
void symv_launch_one_packed(const SymvPlan& sy, const SymvPacked& pk, const float* v0, const float* v1, const int* skip, hipStream_t st, Gate gate,
                            unsigned long long* early, Extra extra = Extra(), hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr) {
    SymvVerdict vd;
    vd.early = early;
    const SymvArgs a = sy.args(nullptr, 0, v0, v1, skip, vd);
    const SymvPackedSrc src = pk.src();
    const bool timed = ev_start != nullptr || ev_stop != nullptr;
    if (pk.nt) {
        if (!timed) hipLaunchKernelGGL((symv1_packed_kernel<Gate, Extra, true>), dim3(sy.ntiles + 1), dim3(kSyThreads), 0, st, a, src, gate, extra);
        else hipExtLaunchKernelGGL((symv1_packed_kernel<Gate, Extra, true>), dim3(sy.ntiles + 1), dim3(kSyThreads), 0, st, ev_start, ev_stop, 0, a, src, gate, extra);
        return;
    }
    if (!timed) hipLaunchKernelGGL((symv1_packed_kernel<Gate, Extra>), dim3(sy.ntiles + 1), dim3(kSyThreads), 0, st, a, src, gate, extra);
    else hipExtLaunchKernelGGL((symv1_packed_kernel<Gate, Extra>), dim3(sy.ntiles + 1), dim3(kSyThreads), 0, st, ev_start, ev_stop, 0, a, src, gate, extra);
}

// y_i of both right-hand sides from the partial arrays.  NL lanes (a power of two <= 64, consecutive lanes of one
// wave, `sub` = this lane's index among them) share element i: each issues up to 16 partial loads per array at once
// (one memory round trip up to 16 * NL partials), then the lanes combine with shuffles.  The summation order is
// fixed, so the result is bit-reproducible; every lane of the group returns the total.  Used by the tall tail
// kernel (lasso_tall.hip), by the row-sharded x-update (tall_shard.hip) and by the test hook admm_hip_test_symv.
template <int NL, typename T = float>
__device__ __forceinline__ void symv_sum_partials(const T* __restrict__ dot0, const T* __restrict__ dot1,
                                                  const T* __restrict__ axp0, const T* __restrict__ axp1,
                                                  long long ldo, int nrb, const SymvSched sched, int p32, int i, int sub, bool valid, T& a, T& b) {
    // Branch-free requests: every slot loads from a clamped (always valid) address and out-of-range slots are replaced by
    // zero afterwards, so the 32 loads of a pass are issued back to back.  (The round-2 form guarded each load by two range
    // tests: ~25 instructions of exec-mask bookkeeping per load, ~2 us of issue time in the tall tail kernel before the
    // last request left.)  Offsets fit 32 bits: (nrb + ncb) * ldo < 2^31 up to p ~ 5e5, far beyond what a p x p matrix allows.
    const int ic = valid ? i : 0;
    const int rbi = ic / kSyRB;
    const int rb0 = rbi;                                                // first row strip whose segments reach column ic
    const int ndot = nrb - rb0;
    const int nax = sched.nseg(rbi, p32);                               // segments of row strip rbi (up to its diagonal block)
    const int ntot = valid ? ndot + nax : 0;
    const unsigned ld = (unsigned)ldo;
    a = T(0); b = T(0);
    for (int k0 = 0; k0 < ntot; k0 += 16 * NL) {
        T va[16], vb[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int k = k0 + j * NL + sub;
            const bool isdot = k < ndot;
            const int row = isdot ? rb0 + k : min(k, ntot - 1) - ndot;      // clamped into the axpy rows when k >= ntot
            const unsigned o = (unsigned)row * ld + (unsigned)ic;
            va[j] = (isdot ? dot0 : axp0)[o];
            vb[j] = (isdot ? dot1 : axp1)[o];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const bool in = k0 + j * NL + sub < ntot;
            a += in ? va[j] : T(0); b += in ? vb[j] : T(0);
        }
    }
#pragma unroll
    for (int m = 1; m < NL; m <<= 1) { a += __shfl_xor(a, m, 64); b += __shfl_xor(b, m, 64); }
}

// The same for plane 0 alone (symv1_lower_kernel writes no other): symv_sum_partials' slots, clamping, order and lane combine for `a`,
// so the sum has the bits that function returns as a (or, for the same partials in plane 1, as b) -- at 16 loads per lane, not 32.
// Round 11: `behind` is called once, behind the first 16 requests and ahead of their first use, by every lane with valid == true (the
// only lanes that request anything): the caller's own loads go there -- the tall tail's element loads -- so that they and the partials
// are ONE round trip.  The partials go first because their addresses take the longer arithmetic: formed while the caller's loads are
// pending, a 64-bit multiply-add read a register pair whose upper half was a pending load's destination, and the wait for that load
// stood in front of all sixteen requests.
struct SymvNothingBehind { __device__ __forceinline__ void operator()() const {} };
template <int NL, typename T = float, typename Behind = SymvNothingBehind>
__device__ __forceinline__ T symv_sum_partials1(const T* __restrict__ dot0, const T* __restrict__ axp0,
                                                long long ldo, int nrb, const SymvSched sched, int p32, int i, int sub, bool valid,
                                                Behind behind = Behind()) {
    const int ic = valid ? i : 0;
    const int rbi = ic / kSyRB;
    const int rb0 = rbi;
    const int ndot = nrb - rb0;
    const int nax = sched.nseg(rbi, p32);
    const int ntot = valid ? ndot + nax : 0;
    const unsigned ld = (unsigned)ldo;
    T a = T(0);
    const auto request = [&](int k0, T (&va)[16]) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int k = k0 + j * NL + sub;
            const bool isdot = k < ndot;
            const int row = isdot ? rb0 + k : min(k, ntot - 1) - ndot;
            const unsigned o = (unsigned)row * ld + (unsigned)ic;
            va[j] = (isdot ? dot0 : axp0)[o];
        }
    };
    const auto add = [&](int k0, const T (&va)[16]) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const bool in = k0 + j * NL + sub < ntot;
            a += in ? va[j] : T(0);
        }
    };
    constexpr bool peel = !std::is_same<Behind, SymvNothingBehind>::value;      // (a caller without loads of its own keeps the plain loop: the tails of the other penalties compile as before)
    if (peel && ntot > 0) {                  // the first pass, peeled for `behind`; the loop goes on where it ends
        T va[16];
        request(0, va);
        __builtin_amdgcn_sched_barrier(0);
        behind();
        __builtin_amdgcn_sched_barrier(0);
        add(0, va);
    }
    for (int k0 = peel ? 16 * NL : 0; k0 < ntot; k0 += 16 * NL) {
        T va[16];
        request(k0, va);
        __builtin_amdgcn_sched_barrier(0);
        add(k0, va);
    }
#pragma unroll
    for (int m = 1; m < NL; m <<= 1) a += __shfl_xor(a, m, 64);
    return a;
}

// Launch of one pass of symvn_lower_kernel over the tiles of `sy` with nr = one of kSyNR right-hand sides per pass.
template <typename Extra>
void symvn_launch(const SymvPlan& sy, int nr, const SymvNArgs& a, hipStream_t st, Extra extra, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr) {
    const dim3 grid(sy.ntiles + 1), block(kSyThreads);
    const bool timed = ev_start != nullptr || ev_stop != nullptr;      // start/stop events time exactly this kernel on its stream (hipExtLaunchKernel)
#define ADMM_SYMVN_LAUNCH(NR, NT)                                                                                                        \
    if (timed) hipExtLaunchKernelGGL((symvn_lower_kernel<NR, Extra, NT>), grid, block, 0, st, ev_start, ev_stop, 0, a, extra);           \
    else hipLaunchKernelGGL((symvn_lower_kernel<NR, Extra, NT>), grid, block, 0, st, a, extra)
#define ADMM_SYMVN_CASE(NR)                                                                                                              \
    case NR:                                                                                                                             \
        if (sy.nt) { ADMM_SYMVN_LAUNCH(NR, true); } else { ADMM_SYMVN_LAUNCH(NR, false); }                                               \
        break;
    switch (nr) {
        ADMM_SYMVN_CASE(2) ADMM_SYMVN_CASE(4) ADMM_SYMVN_CASE(8) ADMM_SYMVN_CASE(12)
        default: throw Error(ADMM_ERR_INTERNAL, "symvn_lower_kernel is not built for that many right-hand sides per pass");
    }
#undef ADMM_SYMVN_CASE
#undef ADMM_SYMVN_LAUNCH
}

// symv_sum_partials for KB consecutive pairs of planes (pair k: dot + 2 k * dot_stride and the plane behind it, the same for axp) with
// the loads of ALL the pairs issued before any is consumed: one memory round trip per 8 NL partials of every pair instead of KB
// dependent ones.  Per pair the additions are symv_sum_partials' in its order (8 slots per step here, 16 there: the running sums take
// the same terms in the same order), so a[k], b[k] are its values to the bit.  Pairs >= npair are not loaded (a = b = 0).
constexpr int kMtChunk = 4;      // the KB of the multi-task tail (lasso_tall.hip, tall_mt_tail_kernel) and of the test hook that walks the pairs as it does
template <int NL, int KB>
__device__ __forceinline__ void symv_sum_partials_n(const float* __restrict__ dot, long long dot_stride, const float* __restrict__ axp, long long axp_stride,
                                                    int npair, long long ldo, int nrb, const SymvSched sched, int p32, int i, int sub, bool valid,
                                                    float (&a)[KB], float (&b)[KB]) {
    const int ic = valid ? i : 0;
    const int rbi = ic / kSyRB;
    const int ndot = nrb - rbi;
    const int nax = sched.nseg(rbi, p32);
    const int ntot = valid ? ndot + nax : 0;
    const unsigned ld = (unsigned)ldo;
#pragma unroll
    for (int k = 0; k < KB; ++k) { a[k] = 0.f; b[k] = 0.f; }
    for (int k0 = 0; k0 < ntot; k0 += 8 * NL) {
        float va[KB][8], vb[KB][8];
#pragma unroll
        for (int k = 0; k < KB; ++k) {
            const int kc = min(k, npair - 1);                                  // clamped: always a valid plane
            const float* d0 = dot + (size_t)(2 * kc) * dot_stride; const float* d1 = d0 + dot_stride;
            const float* x0 = axp + (size_t)(2 * kc) * axp_stride; const float* x1 = x0 + axp_stride;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int s = k0 + j * NL + sub;
                const bool isdot = s < ndot;
                const int row = isdot ? rbi + s : min(s, ntot - 1) - ndot;
                const unsigned o = (unsigned)row * ld + (unsigned)ic;
                va[k][j] = (isdot ? d0 : x0)[o];
                vb[k][j] = (isdot ? d1 : x1)[o];
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < KB; ++k) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bool in = k0 + j * NL + sub < ntot && k < npair;
                a[k] += in ? va[k][j] : 0.f; b[k] += in ? vb[k][j] : 0.f;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < KB; ++k) {
#pragma unroll
        for (int m = 1; m < NL; m <<= 1) { a[k] += __shfl_xor(a[k], m, 64); b[k] += __shfl_xor(b[k], m, 64); }
    }
}

}  // namespace admm
