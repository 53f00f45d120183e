// Test hooks behind the C ABI (include/admm_hip.h, "test hooks"): single kernels of the solvers run on caller data so
// that the test-suite can compare them with the oracle / NumPy.  No solver entry point calls anything in this file.
#include "symv_kernels.h"
#include "prep.h"
#include "gather_kernels.h"
#include "gemv_kernels.h"
#include "test_hooks.h"
#include <cstring>
#include <limits>
#include <vector>

namespace admm {
void require_device();

// The consumer side of the symmetric mat-vec, with the tall tail kernel's geometry and summation order
// (kSySumLanes lanes per element, 256 threads per workgroup).
__global__ void __launch_bounds__(256)
test_symv_finish_kernel(const float* dot0, const float* dot1, const float* axp0, const float* axp1, long long ldo, int nrb, SymvSched sched, int p32,
                        int p, float* y0, float* y1) {
    const int sub = threadIdx.x & (kSySumLanes - 1);
    const int i = blockIdx.x * (256 / kSySumLanes) + threadIdx.x / kSySumLanes;
    float a, b;
    symv_sum_partials<kSySumLanes>(dot0, dot1, axp0, axp1, ldo, nrb, sched, p32, i, sub, i < p, a, b);
    if (i < p && sub == 0) { y0[i] = a; y1[i] = b; }
}

void test_symv(const float* A, int p, const float* v0, const float* v1, float* y0, float* y1) {
    require_device();
    Stream st;
    const long long lda = round_up(p, 128), ldv = round_up(p, 256);      // the tall plan's storage (lasso_tall.hip)
    DevBuf<float> dA((size_t)lda * lda), d0(ldv), d1(ldv), o0(ldv), o1(ldv);
    dA.zero(st.s); d0.zero(st.s); d1.zero(st.s);
    ADMM_HIP_CHECK(hipMemcpy2DAsync(dA.get(), lda * sizeof(float), A, (size_t)p * sizeof(float), (size_t)p * sizeof(float), p,
                                    hipMemcpyHostToDevice, st.s));
    ADMM_HIP_CHECK(hipMemcpyAsync(d0.get(), v0, (size_t)p * sizeof(float), hipMemcpyHostToDevice, st.s));
    ADMM_HIP_CHECK(hipMemcpyAsync(d1.get(), v1, (size_t)p * sizeof(float), hipMemcpyHostToDevice, st.s));
    SymvPlan sy;
    sy.init(p, st.s);
    sy.launch(dA.get(), lda, d0.get(), d1.get(), nullptr, st.s);
    const int per = 256 / kSySumLanes;
    hipLaunchKernelGGL(test_symv_finish_kernel, dim3((p + per - 1) / per), dim3(256), 0, st.s, sy.dot0.get(), sy.dot1.get(),
                       sy.axp0.get(), sy.axp1.get(), sy.ldo, sy.nrb, sy.sched, sy.p32, p, o0.get(), o1.get());
    ADMM_HIP_CHECK(hipGetLastError());
    ADMM_HIP_CHECK(hipMemcpyAsync(y0, o0.get(), (size_t)p * sizeof(float), hipMemcpyDeviceToHost, st.s));
    ADMM_HIP_CHECK(hipMemcpyAsync(y1, o1.get(), (size_t)p * sizeof(float), hipMemcpyDeviceToHost, st.s));
    st.sync();
}

// The multi-vector kernel of the multi-task lasso (symvn_lower_kernel) on nr vectors V [nr][p], rhs_per_pass of them per pass over the
// triangle, with the plan's storage: planes of right-hand sides and of partials, summed by symv_sum_partials pair by pair
// (vectors 2k, 2k + 1 are the pair of "response" k; an odd nr gets a zero vector behind it).
__global__ void __launch_bounds__(256)
test_symvn_finish_kernel(const float* dot, long long dot_stride, const float* axp, long long axp_stride, long long ldo, int nrb, SymvSched sched, int p32,
                         int p, int npair, float* y, long long ldy) {
    const int sub = threadIdx.x & (kSySumLanes - 1);
    const int i = blockIdx.x * (256 / kSySumLanes) + threadIdx.x / kSySumLanes;
    for (int k = 0; k < npair; ++k) {
        float a, b;
        symv_sum_partials<kSySumLanes>(dot + (size_t)(2 * k) * dot_stride, dot + (size_t)(2 * k + 1) * dot_stride,
                                       axp + (size_t)(2 * k) * axp_stride, axp + (size_t)(2 * k + 1) * axp_stride, ldo, nrb, sched, p32, i, sub, i < p, a, b);
        if (i < p && sub == 0) { y[(size_t)(2 * k) * ldy + i] = a; y[(size_t)(2 * k + 1) * ldy + i] = b; }
    }
}

void test_symv_multi(const float* A, int p, const float* V, int nr, int rhs_per_pass, float* Yout) {
    bool built = false;
    for (int k = 0; k < kSyNRCount; ++k) built = built || kSyNR[k] == rhs_per_pass;
    ADMM_REQUIRE(built, "rhs_per_pass must be one of the built widths (2, 4, 8, 12)");
    require_device();
    Stream st;
    const long long lda = round_up(p, 128), ldv = round_up(p, 256);
    const int nv = (nr + 1) / 2 * 2;
    DevBuf<float> dA((size_t)lda * lda), dV((size_t)nv * ldv), dY((size_t)nv * ldv);
    dA.zero(st.s); dV.zero(st.s);
    ADMM_HIP_CHECK(hipMemcpy2DAsync(dA.get(), lda * sizeof(float), A, (size_t)p * sizeof(float), (size_t)p * sizeof(float), p,
                                    hipMemcpyHostToDevice, st.s));
    ADMM_HIP_CHECK(hipMemcpy2DAsync(dV.get(), ldv * sizeof(float), V, (size_t)p * sizeof(float), (size_t)p * sizeof(float), nr,
                                    hipMemcpyHostToDevice, st.s));
    SymvPlan sy;
    sy.init(p, st.s);
    const size_t ds = (size_t)sy.nrb * sy.ldo, as = (size_t)sy.nax_rows * sy.ldo;
    DevBuf<float> dot((size_t)nv * ds), axp((size_t)nv * as);
    dot.zero(st.s); axp.zero(st.s);
    for (int r0 = 0; r0 < nv; r0 += rhs_per_pass) {
        SymvNArgs a;
        a.A = dA.get(); a.lda = lda; a.p = p;
        a.v = dV.get() + (size_t)r0 * ldv; a.vstride = ldv;
        a.dot = dot.get() + (size_t)r0 * ds; a.dot_stride = (long long)ds;
        a.axp = axp.get() + (size_t)r0 * as; a.axp_stride = (long long)as;
        a.nvec = std::min(rhs_per_pass, nv - r0); a.ldo = sy.ldo; a.tiles = sy.tiles.get(); a.skip = nullptr;
        symvn_launch(sy, rhs_per_pass, a, st.s, SymvNoExtra());
    }
    const int per = 256 / kSySumLanes;
    hipLaunchKernelGGL(test_symvn_finish_kernel, dim3((p + per - 1) / per), dim3(256), 0, st.s, dot.get(), (long long)ds, axp.get(), (long long)as,
                       sy.ldo, sy.nrb, sy.sched, sy.p32, p, nv / 2, dY.get(), ldv);
    ADMM_HIP_CHECK(hipGetLastError());
    ADMM_HIP_CHECK(hipMemcpy2DAsync(Yout, (size_t)p * sizeof(float), dY.get(), ldv * sizeof(float), (size_t)p * sizeof(float), nr,
                                    hipMemcpyDeviceToHost, st.s));
    st.sync();
}

// ---- every variant of the symmetric x-update under every tile schedule (tests/test_gpu_symv_variants.py).  The three hooks below
// use the tall plan's storage (lda = round_up(p, 128), vectors zero padded to 256), the plan's own tile list and partial arrays, and
// report the schedule the plan used (sched_out: width_big, width_small, rb_split) so that a test can assert which class it ran.

static void report_sched(const SymvSched& sc, int* sched_out) {
    sched_out[0] = sc.width_big; sched_out[1] = sc.width_small; sched_out[2] = sc.rb_split;
}

bool test_symv_rhs_built(int rhs_per_pass) {
    for (int k = 0; k < kSyNRCount; ++k) if (kSyNR[k] == rhs_per_pass) return true;
    return false;
}

// The host half of SymvPlan::init alone (symv_plan_layout): no device.  info_out: nrb, p32, ldo, nax_rows, nt, number of tiles;
// tiles_out: (row block, first column, width, segment) of every tile, in launch order.
void test_symv_plan(int p, int cus, int part, int nparts, int* sched_out, long long* info_out, int* tiles_out, int tile_capacity) {
    const SymvLayout L = symv_plan_layout(p, cus <= 0 ? 256 : cus, part, nparts);
    ADMM_REQUIRE((long long)L.tiles.size() <= (long long)tile_capacity,
                 "symv plan hook: tile_capacity is too small for the " + std::to_string(L.tiles.size()) + " tiles of this plan");
    report_sched(L.sched, sched_out);
    info_out[0] = L.nrb; info_out[1] = L.p32; info_out[2] = L.ldo; info_out[3] = L.nax_rows; info_out[4] = L.nt ? 1 : 0; info_out[5] = (long long)L.tiles.size();
    for (size_t k = 0; k < L.tiles.size(); ++k) {
        const int4 t = L.tiles[k];
        tiles_out[4 * k + 0] = t.x; tiles_out[4 * k + 1] = t.y; tiles_out[4 * k + 2] = t.z; tiles_out[4 * k + 3] = t.w;
    }
}

// symv2_lower_kernel, one chosen instantiation (variant 0 plain, 1 non-temporal, 2 with the mid-tile verdict check) over the tiles of
// rank `part` of `nparts`, into the plan's zeroed partial arrays, and the usual consumer.  The verdict of variant 2 is the plan's zero
// words with discard = ~0: no tile can leave, so the count of early exits must come back 0.
void test_symv_ex(const float* A, int p, const float* v0, const float* v1, int variant, int part, int nparts, float* y0, float* y1, int* sched_out) {
    require_device();
    Stream st;
    const long long lda = round_up(p, 128), ldv = round_up(p, 256);
    DevBuf<float> dA((size_t)lda * lda), d0(ldv), d1(ldv), o0(ldv), o1(ldv);
    DevBuf<unsigned long long> early(1);
    dA.zero(st.s); d0.zero(st.s); d1.zero(st.s); early.zero(st.s);
    ADMM_HIP_CHECK(hipMemcpy2DAsync(dA.get(), lda * sizeof(float), A, (size_t)p * sizeof(float), (size_t)p * sizeof(float), p,
                                    hipMemcpyHostToDevice, st.s));
    ADMM_HIP_CHECK(hipMemcpyAsync(d0.get(), v0, (size_t)p * sizeof(float), hipMemcpyHostToDevice, st.s));
    ADMM_HIP_CHECK(hipMemcpyAsync(d1.get(), v1, (size_t)p * sizeof(float), hipMemcpyHostToDevice, st.s));
    SymvPlan sy;
    sy.init(p, st.s, part, nparts);
    report_sched(sy.sched, sched_out);
    sy.nt = variant == 1;                      // launch() takes the non-temporal instantiation on this flag alone
    SymvVerdict vd;
    if (variant == 2) { vd.words = sy.zero.get(); vd.discard = ~0ull; vd.early = early.get(); vd.mid = true; }
    sy.launch(dA.get(), lda, d0.get(), d1.get(), nullptr, st.s, SymvNoExtra(), nullptr, nullptr, vd);
    ADMM_HIP_CHECK(hipGetLastError());
    const int per = 256 / kSySumLanes;
    hipLaunchKernelGGL(test_symv_finish_kernel, dim3((p + per - 1) / per), dim3(256), 0, st.s, sy.dot0.get(), sy.dot1.get(),
                       sy.axp0.get(), sy.axp1.get(), sy.ldo, sy.nrb, sy.sched, sy.p32, p, o0.get(), o1.get());
    ADMM_HIP_CHECK(hipGetLastError());
    unsigned long long left = 0;
    ADMM_HIP_CHECK(hipMemcpyAsync(y0, o0.get(), (size_t)p * sizeof(float), hipMemcpyDeviceToHost, st.s));
    ADMM_HIP_CHECK(hipMemcpyAsync(y1, o1.get(), (size_t)p * sizeof(float), hipMemcpyDeviceToHost, st.s));
    ADMM_HIP_CHECK(hipMemcpyAsync(&left, early.get(), sizeof(left), hipMemcpyDeviceToHost, st.s));
    st.sync();
    if (left != 0)
        throw Error(ADMM_ERR_INTERNAL, std::to_string(left) + " tiles left early on a verdict word that cannot equal `discard`");
}

// symv1_lower_kernel (the decide-first x-update's one-vector kernel) with a forced gate, on the plan's storage: gate 0 / 1 multiplies v0 / v1
// into plane 0, 2 leaves (every tile counted, nothing written); 3 runs symv2_lower_kernel on the same storage instead, the reference of the
// bit-identity tests.  Both planes of partials are pre-filled with the 32-bit pattern `fill` and handed back as they are afterwards.
// y[0]: plane 0 through the one-plane sum of TAIL_SYMV1 (symv_sum_partials1); gate 3: y[0], y[1] = the two-plane sum's a, b.
__global__ void __launch_bounds__(256)
test_symv_finish_one_kernel(const float* dot0, const float* axp0, long long ldo, int nrb, SymvSched sched, int p32, int p, float* y0) {
    const int sub = threadIdx.x & (kSySumLanes - 1);
    const int i = blockIdx.x * (256 / kSySumLanes) + threadIdx.x / kSySumLanes;
    const float a = symv_sum_partials1<kSySumLanes>(dot0, axp0, ldo, nrb, sched, p32, i, sub, i < p);
    if (i < p && sub == 0) y0[i] = a;
}

void test_symv_one(const float* A, int p, const float* v0, const float* v1, int gate, int nt, unsigned fill, float* y, float* dot_out, float* axp_out,
                   long long plane_capacity, long long* info_out, int* sched_out) {
    require_device();
    Stream st;
    const long long lda = round_up(p, 128), ldv = round_up(p, 256);
    DevBuf<float> dA((size_t)lda * lda), d0(ldv), d1(ldv), o0(ldv), o1(ldv);
    DevBuf<unsigned long long> early((size_t)kSyEarlySlots * kSyVerdictStride);
    dA.zero(st.s); d0.zero(st.s); d1.zero(st.s); early.zero(st.s);
    ADMM_HIP_CHECK(hipMemcpy2DAsync(dA.get(), lda * sizeof(float), A, (size_t)p * sizeof(float), (size_t)p * sizeof(float), p,
                                    hipMemcpyHostToDevice, st.s));
    ADMM_HIP_CHECK(hipMemcpyAsync(d0.get(), v0, (size_t)p * sizeof(float), hipMemcpyHostToDevice, st.s));
    ADMM_HIP_CHECK(hipMemcpyAsync(d1.get(), v1, (size_t)p * sizeof(float), hipMemcpyHostToDevice, st.s));
    SymvPlan sy;
    sy.init(p, st.s);
    report_sched(sy.sched, sched_out);
    const size_t nd = (size_t)sy.nrb * sy.ldo, na = (size_t)sy.nax_rows * sy.ldo;
    info_out[0] = sy.ntiles; info_out[1] = -1; info_out[2] = (long long)nd; info_out[3] = (long long)na;
    ADMM_REQUIRE(dot_out == nullptr || (long long)std::max(nd, na) <= plane_capacity,
                 "symv_one hook: plane_capacity is too small for the " + std::to_string(std::max(nd, na)) + " floats of a plane of partials");
    sy.nt = nt != 0;
    float* planes[4] = {sy.dot0.get(), sy.dot1.get(), sy.axp0.get(), sy.axp1.get()};
    for (int k = 0; k < 4; ++k) ADMM_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(planes[k]), (int)fill, k < 2 ? nd : na, st.s));
    const int per = 256 / kSySumLanes;
    if (gate == 3) {
        sy.launch(dA.get(), lda, d0.get(), d1.get(), nullptr, st.s);
        hipLaunchKernelGGL(test_symv_finish_kernel, dim3((p + per - 1) / per), dim3(256), 0, st.s, sy.dot0.get(), sy.dot1.get(),
                           sy.axp0.get(), sy.axp1.get(), sy.ldo, sy.nrb, sy.sched, sy.p32, p, o0.get(), o1.get());
    } else {
        sy.launch_one(dA.get(), lda, d0.get(), d1.get(), nullptr, st.s, SymvForcedGate{gate == 2 ? kSyGateLeave : gate}, early.get());
        hipLaunchKernelGGL(test_symv_finish_one_kernel, dim3((p + per - 1) / per), dim3(256), 0, st.s, sy.dot0.get(), sy.axp0.get(),
                           sy.ldo, sy.nrb, sy.sched, sy.p32, p, o0.get());
    }
    ADMM_HIP_CHECK(hipGetLastError());
    std::vector<unsigned long long> slots((size_t)kSyEarlySlots * kSyVerdictStride);
    ADMM_HIP_CHECK(hipMemcpyAsync(y, o0.get(), (size_t)p * sizeof(float), hipMemcpyDeviceToHost, st.s));
    if (gate == 3) ADMM_HIP_CHECK(hipMemcpyAsync(y + p, o1.get(), (size_t)p * sizeof(float), hipMemcpyDeviceToHost, st.s));
    ADMM_HIP_CHECK(hipMemcpyAsync(slots.data(), early.get(), slots.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st.s));
    if (dot_out != nullptr) {
        for (int k = 0; k < 2; ++k) {
            ADMM_HIP_CHECK(hipMemcpyAsync(dot_out + (size_t)k * plane_capacity, planes[k], nd * sizeof(float), hipMemcpyDeviceToHost, st.s));
            ADMM_HIP_CHECK(hipMemcpyAsync(axp_out + (size_t)k * plane_capacity, planes[2 + k], na * sizeof(float), hipMemcpyDeviceToHost, st.s));
        }
    }
    st.sync();
    long long left = 0;
    for (int k = 0; k < kSyEarlySlots; ++k) left += (long long)slots[(size_t)k * kSyVerdictStride];
    info_out[1] = left;
}

// The 29-bit record format (symv_pack.h) on the host alone: bits [nchunks][64][32] (lane-major records of 32 entries) are encoded against
// *base_io (negative: the largest upper-seven-bit exponent among the finite non-zero entries, handed back) into stream_out
// [nchunks][1856] dwords in the memory layout of a wave's chunk; escapes go to esc_out as (chunk << 11 | lane << 5 | entry, bits) while
// they fit esc_cap and are all counted in *nesc_out; decoded_out [nchunks][64][32]: the stream decoded again (escapes as +0.0).
void test_symv_pack_host(const unsigned* bits, int nchunks, int* base_io, unsigned* stream_out, unsigned* esc_out, int esc_cap, long long* nesc_out,
                         unsigned* decoded_out) {
    const size_t n = (size_t)nchunks * 64 * kSpEntries;
    int base = *base_io;
    if (base < 0) {
        base = 0;
        for (size_t k = 0; k < n; ++k) if (sp_counts(bits[k])) base = std::max(base, sp_exp7(bits[k]));
        *base_io = base;
    }
    long long met = 0;
    for (int c = 0; c < nchunks; ++c) {
        for (int lane = 0; lane < 64; ++lane) {
            unsigned in[kSpEntries], rec[kSpRecDwords], out[kSpEntries];
            const size_t at = ((size_t)c * 64 + lane) * kSpEntries;
            for (int e = 0; e < kSpEntries; ++e) in[e] = bits[at + e];
            const unsigned em = sp_record_encode(in, base, rec);
            for (int j = 0; j < kSpRecDwords; ++j) stream_out[(size_t)c * kSpChunkDwords + sp_dword_pos(lane, j)] = rec[j];
            for (int e = 0; e < kSpEntries; ++e) {
                if (((em >> e) & 1u) == 0u) continue;
                if (met < esc_cap) { esc_out[2 * met] = ((unsigned)c << 11) | ((unsigned)lane << 5) | (unsigned)e; esc_out[2 * met + 1] = in[e]; }
                ++met;
            }
            unsigned back[kSpRecDwords];
            for (int j = 0; j < kSpRecDwords; ++j) back[j] = stream_out[(size_t)c * kSpChunkDwords + sp_dword_pos(lane, j)];
            sp_record_decode(back, base, out);
            for (int k = 0; k < 8; ++k) {              // the byte-wise decode against the format as it is stated, entry by entry
                unsigned plain[4];
                sp_column_decode_plain(back[k >> 1], back[4 + 3 * k], back[5 + 3 * k], back[6 + 3 * k], back[28], k, base, plain);
                for (int cc = 0; cc < 4; ++cc)
                    if (plain[cc] != out[4 * k + cc]) throw Error(ADMM_ERR_INTERNAL, "symv_pack_host hook: the two decodes of a record disagree");
            }
            for (int e = 0; e < kSpEntries; ++e) decoded_out[at + e] = out[e];
        }
    }
    *nesc_out = met;
}

// test_symv_one's storage and read-out for symv1_packed_kernel: the plan's tiles are packed (escape lists of esc_cap entries) and the forced gate
// runs on the packed copy.  info_out[8]: tiles, tiles that left, floats of a dot / axpy plane, escapes met, tiles whose list overflowed,
// bytes of the packed stream, 1 if the packed kernel ran (an overflow leaves the planes as filled and this 0).
void test_symv_packed(const float* A, int p, const float* v0, const float* v1, int gate, int nt, unsigned fill, int esc_cap, float* y, float* dot_out,
                      float* axp_out, long long plane_capacity, long long* info_out, int* sched_out) {
    require_device();
    Stream st;
    const long long lda = round_up(p, 128), ldv = round_up(p, 256);
    DevBuf<float> dA((size_t)lda * lda), d0(ldv), d1(ldv), o0(ldv);
    DevBuf<unsigned long long> early((size_t)kSyEarlySlots * kSyVerdictStride);
    dA.zero(st.s); d0.zero(st.s); d1.zero(st.s); o0.zero(st.s); early.zero(st.s);
    ADMM_HIP_CHECK(hipMemcpy2DAsync(dA.get(), lda * sizeof(float), A, (size_t)p * sizeof(float), (size_t)p * sizeof(float), p,
                                    hipMemcpyHostToDevice, st.s));
    ADMM_HIP_CHECK(hipMemcpyAsync(d0.get(), v0, (size_t)p * sizeof(float), hipMemcpyHostToDevice, st.s));
    ADMM_HIP_CHECK(hipMemcpyAsync(d1.get(), v1, (size_t)p * sizeof(float), hipMemcpyHostToDevice, st.s));
    SymvPlan sy;
    sy.init(p, st.s);
    report_sched(sy.sched, sched_out);
    const size_t nd = (size_t)sy.nrb * sy.ldo, na = (size_t)sy.nax_rows * sy.ldo;
    info_out[0] = sy.ntiles; info_out[1] = -1; info_out[2] = (long long)nd; info_out[3] = (long long)na;
    ADMM_REQUIRE(dot_out == nullptr || (long long)std::max(nd, na) <= plane_capacity,
                 "symv_packed hook: plane_capacity is too small for the " + std::to_string(std::max(nd, na)) + " floats of a plane of partials");
    float* planes[4] = {sy.dot0.get(), sy.dot1.get(), sy.axp0.get(), sy.axp1.get()};
    for (int k = 0; k < 4; ++k) ADMM_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(planes[k]), (int)fill, k < 2 ? nd : na, st.s));
    SymvPacked pk;
    const bool ok = pk.build(sy, dA.get(), lda, st.s, esc_cap);
    info_out[4] = (long long)pk.escapes; info_out[5] = (long long)pk.overflowed; info_out[6] = (long long)pk.bytes(); info_out[7] = ok ? 1 : 0;
    pk.nt = nt != 0;
    const int per = 256 / kSySumLanes;
    if (ok) {
        symv_launch_one_packed(sy, pk, d0.get(), d1.get(), nullptr, st.s, SymvForcedGate{gate == 2 ? kSyGateLeave : gate}, early.get());
        hipLaunchKernelGGL(test_symv_finish_one_kernel, dim3((p + per - 1) / per), dim3(256), 0, st.s, sy.dot0.get(), sy.axp0.get(),
                           sy.ldo, sy.nrb, sy.sched, sy.p32, p, o0.get());
    }
    ADMM_HIP_CHECK(hipGetLastError());
    std::vector<unsigned long long> slots((size_t)kSyEarlySlots * kSyVerdictStride);
    ADMM_HIP_CHECK(hipMemcpyAsync(y, o0.get(), (size_t)p * sizeof(float), hipMemcpyDeviceToHost, st.s));
    ADMM_HIP_CHECK(hipMemcpyAsync(slots.data(), early.get(), slots.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st.s));
    if (dot_out != nullptr) {
        for (int k = 0; k < 2; ++k) {
            ADMM_HIP_CHECK(hipMemcpyAsync(dot_out + (size_t)k * plane_capacity, planes[k], nd * sizeof(float), hipMemcpyDeviceToHost, st.s));
            ADMM_HIP_CHECK(hipMemcpyAsync(axp_out + (size_t)k * plane_capacity, planes[2 + k], na * sizeof(float), hipMemcpyDeviceToHost, st.s));
        }
    }
    st.sync();
    long long left = 0;
    for (int k = 0; k < kSyEarlySlots; ++k) left += (long long)slots[(size_t)k * kSyVerdictStride];
    info_out[1] = left;
}

// The bare tile loops against each other, event-timed launch by launch (scripts/symv_packed_gate.py): us_out [4][reps] = fp32 / packed after
// a pass over a buffer larger than the Infinity Cache ("cold"), fp32 / packed replayed back to back (two launches of warm-up per block, two
// alternating blocks of reps / 2 each).  info_out[4]: tiles, escapes met, tiles overflowed, bytes of the packed stream.
void test_symv_packed_time(const float* A, int p, const float* v0, int reps, float* us_out, long long* info_out) {
    require_device();
    Stream st;
    const long long lda = round_up(p, 128), ldv = round_up(p, 256);
    DevBuf<float> dA((size_t)lda * lda), d0(ldv);
    DevBuf<unsigned long long> early((size_t)kSyEarlySlots * kSyVerdictStride);
    DevBuf<unsigned> flush((size_t)192 << 20);      // 768 MB
    dA.zero(st.s); d0.zero(st.s); early.zero(st.s);
    ADMM_HIP_CHECK(hipMemcpy2DAsync(dA.get(), lda * sizeof(float), A, (size_t)p * sizeof(float), (size_t)p * sizeof(float), p,
                                    hipMemcpyHostToDevice, st.s));
    ADMM_HIP_CHECK(hipMemcpyAsync(d0.get(), v0, (size_t)p * sizeof(float), hipMemcpyHostToDevice, st.s));
    SymvPlan sy;
    sy.init(p, st.s);
    SymvPacked pk;
    const bool ok = pk.build(sy, dA.get(), lda, st.s);
    info_out[0] = sy.ntiles; info_out[1] = (long long)pk.escapes; info_out[2] = (long long)pk.overflowed; info_out[3] = (long long)pk.bytes();
    ADMM_REQUIRE(ok, "symv_packed_time hook: a tile's escape list overflowed");
    hipEvent_t e0, e1;
    ADMM_HIP_CHECK(hipEventCreate(&e0)); ADMM_HIP_CHECK(hipEventCreate(&e1));
    const SymvForcedGate gate{0};
    const auto one = [&](int kind, bool timed) {
        float ms = 0.f;
        if (kind == 0) sy.launch_one(dA.get(), lda, d0.get(), d0.get(), nullptr, st.s, gate, early.get(), SymvNoExtra(), timed ? e0 : nullptr, timed ? e1 : nullptr);
        else symv_launch_one_packed(sy, pk, d0.get(), d0.get(), nullptr, st.s, gate, early.get(), SymvNoExtra(), timed ? e0 : nullptr, timed ? e1 : nullptr);
        ADMM_HIP_CHECK(hipGetLastError());
        if (timed) { ADMM_HIP_CHECK(hipEventSynchronize(e1)); ADMM_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1)); }
        return ms * 1000.f;
    };
    for (int r = 0; r < reps; ++r) {
        for (int kind = 0; kind < 2; ++kind) {
            ADMM_HIP_CHECK(hipMemsetAsync(flush.get(), r + kind, flush.n * sizeof(unsigned), st.s));
            us_out[(size_t)kind * reps + r] = one(kind, true);
        }
    }
    const int half = reps / 2;
    for (int blk = 0; blk < 2; ++blk) {
        for (int kind = 0; kind < 2; ++kind) {
            one(kind, false); one(kind, false);
            for (int r = 0; r < half; ++r) us_out[(size_t)(2 + kind) * reps + blk * half + r] = one(kind, true);
        }
    }
    st.sync();
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
}

// test_symvn_finish_kernel with the consumer the multi-task tail really uses: symv_sum_partials_n over chunks of kMtChunk pairs, walked
// as tall_mt_tail_kernel walks them (chunk k0: planes from 2 k0, nk = min(kMtChunk, npair - k0) pairs of it valid).
__global__ void __launch_bounds__(256)
test_symvn_finish_chunks_kernel(const float* dot, long long dot_stride, const float* axp, long long axp_stride, long long ldo, int nrb, SymvSched sched,
                                int p32, int p, int npair, float* y, long long ldy) {
    const int sub = threadIdx.x & (kSySumLanes - 1);
    const int i = blockIdx.x * (256 / kSySumLanes) + threadIdx.x / kSySumLanes;
    for (int k0 = 0; k0 < npair; k0 += kMtChunk) {
        const int nk = min(kMtChunk, npair - k0);
        float a[kMtChunk], b[kMtChunk];
        symv_sum_partials_n<kSySumLanes, kMtChunk>(dot + (size_t)(2 * k0) * dot_stride, dot_stride, axp + (size_t)(2 * k0) * axp_stride, axp_stride,
                                                   nk, ldo, nrb, sched, p32, i, sub, i < p, a, b);
#pragma unroll
        for (int kk = 0; kk < kMtChunk; ++kk) {
            if (kk < nk && i < p && sub == 0) { y[(size_t)(2 * (k0 + kk)) * ldy + i] = a[kk]; y[(size_t)(2 * (k0 + kk) + 1) * ldy + i] = b[kk]; }
        }
    }
}

// test_symv_multi with the instantiation (nt) and the consumer (finish 0: symv_sum_partials pair by pair, 1: symv_sum_partials_n) chosen.
void test_symv_multi_ex(const float* A, int p, const float* V, int nr, int rhs_per_pass, int nt, int finish, float* Yout, int* sched_out) {
    require_device();
    Stream st;
    const long long lda = round_up(p, 128), ldv = round_up(p, 256);
    const int nv = (nr + 1) / 2 * 2;
    DevBuf<float> dA((size_t)lda * lda), dV((size_t)nv * ldv), dY((size_t)nv * ldv);
    dA.zero(st.s); dV.zero(st.s);
    ADMM_HIP_CHECK(hipMemcpy2DAsync(dA.get(), lda * sizeof(float), A, (size_t)p * sizeof(float), (size_t)p * sizeof(float), p,
                                    hipMemcpyHostToDevice, st.s));
    ADMM_HIP_CHECK(hipMemcpy2DAsync(dV.get(), ldv * sizeof(float), V, (size_t)p * sizeof(float), (size_t)p * sizeof(float), nr,
                                    hipMemcpyHostToDevice, st.s));
    SymvPlan sy;
    sy.init(p, st.s);
    report_sched(sy.sched, sched_out);
    sy.nt = nt != 0;                           // symvn_launch takes the non-temporal instantiations on this flag alone
    const size_t ds = (size_t)sy.nrb * sy.ldo, as = (size_t)sy.nax_rows * sy.ldo;
    DevBuf<float> dot((size_t)nv * ds), axp((size_t)nv * as);
    dot.zero(st.s); axp.zero(st.s);
    for (int r0 = 0; r0 < nv; r0 += rhs_per_pass) {
        SymvNArgs a;
        a.A = dA.get(); a.lda = lda; a.p = p;
        a.v = dV.get() + (size_t)r0 * ldv; a.vstride = ldv;
        a.dot = dot.get() + (size_t)r0 * ds; a.dot_stride = (long long)ds;
        a.axp = axp.get() + (size_t)r0 * as; a.axp_stride = (long long)as;
        a.nvec = std::min(rhs_per_pass, nv - r0); a.ldo = sy.ldo; a.tiles = sy.tiles.get(); a.skip = nullptr;
        symvn_launch(sy, rhs_per_pass, a, st.s, SymvNoExtra());
    }
    ADMM_HIP_CHECK(hipGetLastError());
    const int per = 256 / kSySumLanes;
    if (finish == 0)
        hipLaunchKernelGGL(test_symvn_finish_kernel, dim3((p + per - 1) / per), dim3(256), 0, st.s, dot.get(), (long long)ds, axp.get(), (long long)as,
                           sy.ldo, sy.nrb, sy.sched, sy.p32, p, nv / 2, dY.get(), ldv);
    else
        hipLaunchKernelGGL(test_symvn_finish_chunks_kernel, dim3((p + per - 1) / per), dim3(256), 0, st.s, dot.get(), (long long)ds, axp.get(), (long long)as,
                           sy.ldo, sy.nrb, sy.sched, sy.p32, p, nv / 2, dY.get(), ldv);
    ADMM_HIP_CHECK(hipGetLastError());
    ADMM_HIP_CHECK(hipMemcpy2DAsync(Yout, (size_t)p * sizeof(float), dY.get(), ldv * sizeof(float), (size_t)p * sizeof(float), nr,
                                    hipMemcpyDeviceToHost, st.s));
    st.sync();
}

// The refinement's products (lasso_tall.hip): symv2_lower_f64acc_kernel on double partial planes of the plan's shape, summed as
// tall_refine_resid_kernel sums them.
__global__ void __launch_bounds__(256)
test_symv_finish_f64_kernel(const double* dot0, const double* dot1, const double* axp0, const double* axp1, long long ldo, int nrb, SymvSched sched, int p32,
                            int p, double* y0, double* y1) {
    const int sub = threadIdx.x & (kSySumLanes - 1);
    const int i = blockIdx.x * (256 / kSySumLanes) + threadIdx.x / kSySumLanes;
    double a, b;
    symv_sum_partials<kSySumLanes, double>(dot0, dot1, axp0, axp1, ldo, nrb, sched, p32, i, sub, i < p, a, b);
    if (i < p && sub == 0) { y0[i] = a; y1[i] = b; }
}

void test_symv_f64acc(const float* A, int p, const float* v0, const float* v1, double* y0, double* y1, int* sched_out) {
    require_device();
    Stream st;
    const long long lda = round_up(p, 128), ldv = round_up(p, 256);
    DevBuf<float> dA((size_t)lda * lda), d0(ldv), d1(ldv);
    DevBuf<double> o0(ldv), o1(ldv);
    dA.zero(st.s); d0.zero(st.s); d1.zero(st.s);
    ADMM_HIP_CHECK(hipMemcpy2DAsync(dA.get(), lda * sizeof(float), A, (size_t)p * sizeof(float), (size_t)p * sizeof(float), p,
                                    hipMemcpyHostToDevice, st.s));
    ADMM_HIP_CHECK(hipMemcpyAsync(d0.get(), v0, (size_t)p * sizeof(float), hipMemcpyHostToDevice, st.s));
    ADMM_HIP_CHECK(hipMemcpyAsync(d1.get(), v1, (size_t)p * sizeof(float), hipMemcpyHostToDevice, st.s));
    SymvPlan sy;
    sy.init(p, st.s);
    report_sched(sy.sched, sched_out);
    DevBuf<double> dD0((size_t)sy.nrb * sy.ldo), dD1((size_t)sy.nrb * sy.ldo), xD0((size_t)sy.nax_rows * sy.ldo), xD1((size_t)sy.nax_rows * sy.ldo);
    dD0.zero(st.s); dD1.zero(st.s); xD0.zero(st.s); xD1.zero(st.s);
    SymvArgsD ad;
    ad.A = dA.get(); ad.lda = lda; ad.p = p; ad.v0 = d0.get(); ad.v1 = d1.get();
    ad.dot0 = dD0.get(); ad.dot1 = dD1.get(); ad.axp0 = xD0.get(); ad.axp1 = xD1.get(); ad.ldo = sy.ldo; ad.tiles = sy.tiles.get(); ad.skip = nullptr;
    hipLaunchKernelGGL(symv2_lower_f64acc_kernel, dim3(sy.ntiles), dim3(kSyThreads), 0, st.s, ad);
    ADMM_HIP_CHECK(hipGetLastError());
    const int per = 256 / kSySumLanes;
    hipLaunchKernelGGL(test_symv_finish_f64_kernel, dim3((p + per - 1) / per), dim3(256), 0, st.s, dD0.get(), dD1.get(), xD0.get(), xD1.get(),
                       sy.ldo, sy.nrb, sy.sched, sy.p32, p, o0.get(), o1.get());
    ADMM_HIP_CHECK(hipGetLastError());
    ADMM_HIP_CHECK(hipMemcpyAsync(y0, o0.get(), (size_t)p * sizeof(double), hipMemcpyDeviceToHost, st.s));
    ADMM_HIP_CHECK(hipMemcpyAsync(y1, o1.get(), (size_t)p * sizeof(double), hipMemcpyDeviceToHost, st.s));
    st.sync();
}

// Gram matrix through the solvers' own path (gram_full: matrix-core SYRK kernels, split-K for small orders):
// G = A'A (atA) or AA' for a host matrix A (rows x cols, column-major, leading dimension rows); G host, order k, ld k.
template <typename T>
void test_gram(const T* A, int rows, int cols, bool atA, T* G) {
    require_device();
    Stream st;
    const long long lda = round_up(rows, 32);
    const int k = atA ? cols : rows;
    const long long ldc = round_up(k, 128);
    DevBuf<T> dA((size_t)lda * cols), dG((size_t)ldc * ldc);
    dA.zero(st.s); dG.zero(st.s);
    ADMM_HIP_CHECK(hipMemcpy2DAsync(dA.get(), lda * sizeof(T), A, (size_t)rows * sizeof(T), (size_t)rows * sizeof(T), cols, hipMemcpyHostToDevice, st.s));
    gram_full<T>(dA.get(), lda, rows, cols, atA, dG.get(), ldc, st.s);
    ADMM_HIP_CHECK(hipMemcpy2DAsync(G, (size_t)k * sizeof(T), dG.get(), ldc * sizeof(T), (size_t)k * sizeof(T), k, hipMemcpyDeviceToHost, st.s));
    st.sync();
}
template void test_gram<float>(const float*, int, int, bool, float*);
template void test_gram<double>(const double*, int, int, bool, double*);

// y = A' v through the solvers' streaming mat-vec (gemv_t_kernel: contiguous columns, 16 bytes per lane, K-split into row
// segments + ordered partial sums): A host, rows x cols column-major (ld rows), v length rows, y length cols.
template <typename T>
void test_gemv_t(const T* A, int rows, int cols, const T* v, T* y) {
    require_device();
    Stream st;
    const long long lda = round_up(rows, 32), ldy = round_up(cols, 32);
    DevBuf<T> dA((size_t)lda * cols), dv(lda), dy(ldy);
    dA.zero(st.s); dv.zero(st.s); dy.zero(st.s);
    ADMM_HIP_CHECK(hipMemcpy2DAsync(dA.get(), lda * sizeof(T), A, (size_t)rows * sizeof(T), (size_t)rows * sizeof(T), cols, hipMemcpyHostToDevice, st.s));
    ADMM_HIP_CHECK(hipMemcpyAsync(dv.get(), v, (size_t)rows * sizeof(T), hipMemcpyHostToDevice, st.s));
    gemv_t_simple<T>(dA.get(), lda, rows, cols, dv.get(), dy.get(), st.s);
    ADMM_HIP_CHECK(hipMemcpyAsync(y, dy.get(), (size_t)cols * sizeof(T), hipMemcpyDeviceToHost, st.s));
    st.sync();
}
template void test_gemv_t<float>(const float*, int, int, const float*, float*);
template void test_gemv_t<double>(const double*, int, int, const double*, double*);

// ---- every launch form of gemv_t (tests/test_gpu_gemv_family.py): launch_gemv_t with one or two right-hand sides, GemvT::run, the chain
// GemvT::run_partials -> GemvT::run_from, and gemv_t_batch_kernel over argument blocks of different shapes (with a second batched launch
// for the blocks whose right-hand side is the partial rows of a block of the first).  Storage as the callers hold it, but hostile where
// they promise nothing: rows [m, round_up(m, 32)) of a matrix are zero (the callers' contract), every row beyond them and the tail of
// every right-hand vector is NaN, and every partial / output buffer starts as the caller's bit pattern.
template <typename T>
void test_gemv_t_ex(const GemvExRequest& q) {
    require_device();
    Stream st;
    struct Prod {
        GemvT<T> g;
        DevBuf<T> dA, dv, dy;
        long long lda = 0;
        int from = -1, route = 0, vparts = 1, width = 0, nt = 0;
    } P[kGemvHookMaxCount];
    DevBuf<int> dskip(q.count);
    std::vector<int> hskip(q.count, 0);
    std::vector<std::vector<T>> keep;                                 // host staging, alive until the stream has been synchronised
    struct SyncOnExit { hipStream_t s; ~SyncOnExit() { (void)hipStreamSynchronize(s); } } sync_first{st.s};      // (on a refusal too)
    const auto upload = [&](T* dst, std::vector<T>&& h) {
        keep.push_back(std::move(h));
        ADMM_HIP_CHECK(hipMemcpyAsync(dst, keep.back().data(), keep.back().size() * sizeof(T), hipMemcpyHostToDevice, st.s));
    };
    T pattern;
    std::memcpy(&pattern, &q.fill, sizeof(T));                         // (float: the low 32 bits)
    const auto fill = [&](DevBuf<T>& b) { upload(b.get(), std::vector<T>(b.n, pattern)); };
    const T nan = std::numeric_limits<T>::quiet_NaN();
    const size_t cap = (size_t)q.part_capacity;

    for (int i = 0; i < q.count; ++i) {
        Prod& p = P[i];
        const int m = q.m[i], k = q.k[i];
        p.from = q.form == 2 ? (i == 1 ? 0 : -1) : (q.from ? q.from[i] : -1);
        p.lda = round_up(m, 32) + q.lda_extra;
        std::vector<T> hA((size_t)p.lda * k, nan);
        const T* A = static_cast<const T*>(q.A[i]);
        for (int j = 0; j < k; ++j) {
            std::memcpy(&hA[(size_t)j * p.lda], A + (size_t)j * m, (size_t)m * sizeof(T));
            for (long long r = m; r < round_up(m, 32); ++r) hA[(size_t)j * p.lda + r] = T(0);
        }
        p.dA.alloc(hA.size());
        upload(p.dA.get(), std::move(hA));
        if (p.from < 0) {
            std::vector<T> hv((size_t)q.nrhs * p.lda, nan);
            for (int r = 0; r < q.nrhs; ++r) std::memcpy(&hv[(size_t)r * p.lda], static_cast<const T*>(q.v[i]) + (size_t)r * m, (size_t)m * sizeof(T));
            p.dv.alloc(hv.size());
            upload(p.dv.get(), std::move(hv));
        }
        p.g.init(p.dA.get(), p.lda, m, k);                             // (the plan of the solvers' struct, big64 included)
        if (q.form == 0 || q.max_seg_rows > 0) p.g.pl = plan_gemv_t<T>(m, k, q.nrhs, 4, q.max_seg_rows);
        if (q.nt >= 0) p.g.set_nt(q.nt != 0);
        ADMM_REQUIRE((size_t)p.g.pl.nseg * (size_t)p.g.stride <= cap,
                     "gemv_t_ex hook: part_capacity is too small for the " + std::to_string((size_t)p.g.pl.nseg * (size_t)p.g.stride) + " elements of product " +
                         std::to_string(i) + "'s partial rows");
        p.g.part = DevBuf<T>((size_t)q.nrhs * cap);
        p.dy.alloc((size_t)p.g.stride);
        fill(p.g.part); fill(p.dy);
    }
    if (q.skip) hskip.assign(q.skip, q.skip + q.count);
    ADMM_HIP_CHECK(hipMemcpyAsync(dskip.get(), hskip.data(), hskip.size() * sizeof(int), hipMemcpyHostToDevice, st.s));
    for (int i = 0; i < q.count; ++i) {
        Prod& p = P[i];
        p.nt = p.g.pl.nt ? 1 : 0; p.width = p.g.pl.grid;
        if (p.from >= 0) p.vparts = P[p.from].g.pl.nseg;
        p.route = p.vparts > 1 ? 1 : 0;
    }

    if (q.form == 0) {
        Prod& p = P[0];
        T* part = p.g.part.get();
        if (q.nrhs == 1)
            launch_gemv_t<T, 1, 4>(p.g.pl, p.dA.get(), p.lda, p.g.m, p.g.k, p.dv.get(), nullptr, part, nullptr, p.g.stride, dskip.get(), st.s);
        else
            launch_gemv_t<T, 2, 4>(p.g.pl, p.dA.get(), p.lda, p.g.m, p.g.k, p.dv.get(), p.dv.get() + p.lda, part, part + cap, p.g.stride, dskip.get(), st.s);
    } else if (q.form == 1) {
        P[0].g.run(P[0].dv.get(), P[0].dy.get(), dskip.get(), st.s);
    } else if (q.form == 2) {
        Prod& a = P[0];
        Prod& b = P[1];
        if (b.g.pl.nseg > 1 && a.g.pl.nseg > GemvT<T>::kChainRows) {   // the reduce route: its buffer is the struct's, allocated here so that it starts as the pattern
            b.g.red.alloc((size_t)round_up(b.g.m, 32));
            fill(b.g.red);
            b.route = 2;
        }
        a.g.run_partials(a.dv.get(), dskip.get(), st.s);
        b.g.run_from(a.g, b.dy.get(), dskip.get() + 1, st.s);
    } else {
        for (int stage = 0; stage < 2; ++stage) {
            std::vector<GemvTArgs<T>> ha;
            int width = 0, nt = 0;
            size_t lds = 0;
            for (int i = 0; i < q.count; ++i) {
                Prod& p = P[i];
                if ((p.from >= 0) != (stage == 1)) continue;
                ha.push_back(stage == 0 ? p.g.args_partials(p.dv.get(), dskip.get() + i) : p.g.args_partials_from(P[p.from].g, dskip.get() + i));
                width = std::max(width, p.g.pl.grid); lds = std::max(lds, p.g.pl.lds_bytes); nt |= p.g.pl.nt ? 1 : 0;
            }
            if (ha.empty()) continue;
            for (int i = 0; i < q.count; ++i) if ((P[i].from >= 0) == (stage == 1)) { P[i].width = width; P[i].nt = nt; }
            DevBuf<GemvTArgs<T>> dargs(ha.size());
            ADMM_HIP_CHECK(hipMemcpyAsync(dargs.get(), ha.data(), ha.size() * sizeof(GemvTArgs<T>), hipMemcpyHostToDevice, st.s));
            launch_gemv_t_batch<T>(dargs.get(), (int)ha.size(), width, lds, nt != 0, st.s);
            st.sync();                                                 // the argument blocks go out of scope
        }
    }
    ADMM_HIP_CHECK(hipGetLastError());
    for (int i = 0; i < q.count; ++i) {
        Prod& p = P[i];
        ADMM_HIP_CHECK(hipMemcpyAsync(q.part_out[i], p.g.part.get(), (size_t)q.nrhs * cap * sizeof(T), hipMemcpyDeviceToHost, st.s));
        if ((q.form == 1 || q.form == 2) && i == q.count - 1)
            ADMM_HIP_CHECK(hipMemcpyAsync(q.y_out[i], p.dy.get(), (size_t)p.g.stride * sizeof(T), hipMemcpyDeviceToHost, st.s));
        long long* info = q.info_out + 8 * i;
        info[0] = p.g.pl.nseg; info[1] = p.g.pl.seg_len; info[2] = p.g.pl.groups_per_wg; info[3] = p.g.pl.grid; info[4] = p.nt;
        info[5] = p.route; info[6] = p.vparts; info[7] = p.width;
    }
    st.sync();
}
template void test_gemv_t_ex<float>(const GemvExRequest&);
template void test_gemv_t_ex<double>(const GemvExRequest&);

// w = X (X'v) through the wide solver's Gram-free operator (prep.hip: gemv_t_simple, gemv_n_partial_kernel, the ordered sum of its partial
// rows) on the storage DeviceData gives it: leading dimension round_up(n, 32), the padding rows zero.
void test_wide_op(const float* X, int n, int p, const float* v, float* w) {
    require_device();
    Stream st;
    const long long ldx = round_up(n, 32);
    DevBuf<float> dX((size_t)ldx * p);
    dX.zero(st.s);
    ADMM_HIP_CHECK(hipMemcpy2DAsync(dX.get(), ldx * sizeof(float), X, (size_t)n * sizeof(float), (size_t)n * sizeof(float), p, hipMemcpyHostToDevice, st.s));
    GramFreeWideOp op(dX.get(), ldx, n, p, st.s);
    op(v, w);
    st.sync();
    ADMM_HIP_CHECK(hipGetLastError());
}

// y = A v over the non-zeros of v through the gather mat-vec of the one-pass forms (gather_kernels.h): A host, rows x cols
// column-major (ld rows), v length cols, y length rows in DOUBLE (the kernel accumulates in double whatever T is); the column
// groups' partial rows are summed in group order, as the consumers do.
template <typename T>
void test_gather(const T* A, int rows, int cols, const T* v, double* y) {
    require_device();
    Stream st;
    const long long lda = round_up(rows, 32);
    DevBuf<T> dA((size_t)lda * cols), dv(round_up(cols, 32));
    dA.zero(st.s); dv.zero(st.s);
    ADMM_HIP_CHECK(hipMemcpy2DAsync(dA.get(), lda * sizeof(T), A, (size_t)rows * sizeof(T), (size_t)rows * sizeof(T), cols, hipMemcpyHostToDevice, st.s));
    ADMM_HIP_CHECK(hipMemcpyAsync(dv.get(), v, (size_t)cols * sizeof(T), hipMemcpyHostToDevice, st.s));
    const GatherPlan gp = plan_gather<T>(rows, cols);
    DevBuf<double> part((size_t)gp.ngroups * gp.pstride);
    part.zero(st.s);
    const GatherArgs<T> a = gather_args<T>(gp, dA.get(), lda, rows, cols, dv.get(), part.get(), nullptr);
    hipLaunchKernelGGL((gather_kernel<T>), dim3(gp.tiles, gp.ngroups), dim3(kGatherThreads), 0, st.s, a);
    std::vector<double> hp((size_t)gp.ngroups * gp.pstride);
    ADMM_HIP_CHECK(hipMemcpyAsync(hp.data(), part.get(), hp.size() * sizeof(double), hipMemcpyDeviceToHost, st.s));
    st.sync();
    ADMM_HIP_CHECK(hipGetLastError());
    for (int i = 0; i < rows; ++i) {
        double s = 0.0;
        for (int g = 0; g < gp.ngroups; ++g) s += hp[(size_t)g * gp.pstride + i];
        y[i] = s;
    }
}
template void test_gather<float>(const float*, int, int, const float*, double*);
template void test_gather<double>(const double*, int, int, const double*, double*);

// Symmetric inverse of an SPD host matrix (order n, ld n) through the solvers' own path: blocked Cholesky + inverse on
// the matrix cores (chol_inverse.h) for n >= 256.  via64: the float matrix factorised / inverted in double and rounded once.
template <typename T>
void test_spd_inverse(const T* A, int n, T* Ainv, bool via64) {
    require_device();
    Stream st;
    const long long lda = round_up(n, 128);
    DevBuf<T> dA((size_t)lda * lda);
    dA.zero(st.s);
    ADMM_HIP_CHECK(hipMemcpy2DAsync(dA.get(), lda * sizeof(T), A, (size_t)n * sizeof(T), (size_t)n * sizeof(T), n, hipMemcpyHostToDevice, st.s));
    if constexpr (std::is_same<T, float>::value) {
        if (via64) spd_inverse_f32_via_f64(dA.get(), lda, n, 0.0, st.s);
        else spd_inverse_f32(dA.get(), lda, n, st.s);
    } else {
        spd_inverse_f64(dA.get(), lda, n, st.s);
    }
    ADMM_HIP_CHECK(hipMemcpy2DAsync(Ainv, (size_t)n * sizeof(T), dA.get(), lda * sizeof(T), (size_t)n * sizeof(T), n, hipMemcpyDeviceToHost, st.s));
    st.sync();
}
template void test_spd_inverse<float>(const float*, int, float*, bool);
template void test_spd_inverse<double>(const double*, int, double*, bool);

// (A + diag I)^-1 of a float matrix through spd_inverse_f32_via_f64 with the caller's shift (the tall path's rho, added in float).
void test_spd_inverse_shift(const float* A, int n, double diag, float* Ainv) {
    require_device();
    Stream st;
    const long long lda = round_up(n, 128);
    DevBuf<float> dA((size_t)lda * lda);
    dA.zero(st.s);
    ADMM_HIP_CHECK(hipMemcpy2DAsync(dA.get(), lda * sizeof(float), A, (size_t)n * sizeof(float), (size_t)n * sizeof(float), n, hipMemcpyHostToDevice, st.s));
    spd_inverse_f32_via_f64(dA.get(), lda, n, diag, st.s);
    ADMM_HIP_CHECK(hipMemcpy2DAsync(Ainv, (size_t)n * sizeof(float), dA.get(), lda * sizeof(float), (size_t)n * sizeof(float), n, hipMemcpyDeviceToHost, st.s));
    st.sync();
}

// The blocked factorisation alone (chol_inverse.h, cholesky_linvt_blocked through the solvers' launchers): L = the overwritten A
// (order n, ld n: the factor in the lower triangle, the strict upper triangle as the caller gave it) and U = L^-T (order n, ld n).
template <typename T>
void test_cholesky_linvt(const T* A, int n, T* L, T* U) {
    require_device();
    Stream st;
    const long long lda = round_up(n, 128);
    DevBuf<T> dA((size_t)lda * lda);
    dA.zero(st.s);
    ADMM_HIP_CHECK(hipMemcpy2DAsync(dA.get(), lda * sizeof(T), A, (size_t)n * sizeof(T), (size_t)n * sizeof(T), n, hipMemcpyHostToDevice, st.s));
    DevBuf<T> dU;
    if constexpr (std::is_same<T, float>::value) dU = cholesky_linvt_mfma_f32(dA.get(), lda, n, st.s);
    else dU = cholesky_linvt_mfma_f64(dA.get(), lda, n, st.s);
    ADMM_HIP_CHECK(hipMemcpy2DAsync(L, (size_t)n * sizeof(T), dA.get(), lda * sizeof(T), (size_t)n * sizeof(T), n, hipMemcpyDeviceToHost, st.s));
    ADMM_HIP_CHECK(hipMemcpy2DAsync(U, (size_t)n * sizeof(T), dU.get(), lda * sizeof(T), (size_t)n * sizeof(T), n, hipMemcpyDeviceToHost, st.s));
    st.sync();
}
template void test_cholesky_linvt<float>(const float*, int, float*, float*);
template void test_cholesky_linvt<double>(const double*, int, double*, double*);

// One launch of the NT-GEMM of the factorisation / inverse / Gram (syrk_mfma.hip, gemm_f64_mfma.hip): C = alpha A B' + beta C.
// Host operands column-major with the output index contiguous and tight leading dimensions (A: M x K, B: N x K, C: M x N); on the
// device they are stored as the callers keep them: leading dimension round_up(., 128), K padded with zero columns to the K tile.
// in_place: the device copy of A is C as well (the factorisation's U[:, k] <- U[:, k] L_kk^-T: N <= 128, K = 128; the host C is
// only written).  Everything of the device C outside M x N -- a NaN guard band up to the padded storage, or the rest of A when in
// place -- must come back as it was: ADMM_ERR_INTERNAL otherwise.
void test_launch_gemm_nt_f32(bool lower, const float* A, long long lda, const float* B, long long ldb, float* C, long long ldc,
                             int M, int N, int K, float alpha, float beta, bool mirror, bool kstart_row, hipStream_t st);      // syrk_mfma.hip
void test_launch_gemm_nt_f64(bool lower, const double* A, long long lda, const double* B, long long ldb, double* C, long long ldc,
                             int M, int N, int K, double alpha, double beta, bool mirror, bool kstart_row, bool kend_col, hipStream_t st);   // gemm_f64_mfma.hip

template <typename T>
void test_gemm_nt(bool lower, bool mirror, bool kstart_row, bool b_lower, bool in_place, int M, int N, int K, double alpha, double beta,
                  const T* A, const T* B, T* C) {
    require_device();
    Stream st;
    const int Kp = round_up(K, std::is_same<T, float>::value ? 16 : 8);
    const long long lda = round_up(M, 128), ldb = round_up(N, 128), ldc = lda;
    const int ccols = in_place ? Kp : round_up(N, 128);
    std::vector<T> hA((size_t)lda * Kp, T(0)), hB((size_t)ldb * Kp, T(0));
    for (int k = 0; k < K; ++k) {
        std::memcpy(&hA[(size_t)k * lda], A + (size_t)k * M, (size_t)M * sizeof(T));
        std::memcpy(&hB[(size_t)k * ldb], B + (size_t)k * N, (size_t)N * sizeof(T));
    }
    std::vector<T> before;
    if (in_place) before = hA;
    else {
        before.assign((size_t)ldc * ccols, std::numeric_limits<T>::quiet_NaN());
        for (int j = 0; j < N; ++j) std::memcpy(&before[(size_t)j * ldc], C + (size_t)j * M, (size_t)M * sizeof(T));
    }
    DevBuf<T> dA(hA.size()), dB(hB.size()), dC(in_place ? 0 : before.size());
    ADMM_HIP_CHECK(hipMemcpyAsync(dA.get(), hA.data(), hA.size() * sizeof(T), hipMemcpyHostToDevice, st.s));
    ADMM_HIP_CHECK(hipMemcpyAsync(dB.get(), hB.data(), hB.size() * sizeof(T), hipMemcpyHostToDevice, st.s));
    if (!in_place) ADMM_HIP_CHECK(hipMemcpyAsync(dC.get(), before.data(), before.size() * sizeof(T), hipMemcpyHostToDevice, st.s));
    T* out = in_place ? dA.get() : dC.get();
    if constexpr (std::is_same<T, float>::value)
        test_launch_gemm_nt_f32(lower, dA.get(), lda, dB.get(), ldb, out, ldc, M, N, Kp, (float)alpha, (float)beta, mirror, kstart_row, st.s);
    else
        test_launch_gemm_nt_f64(lower, dA.get(), lda, dB.get(), ldb, out, ldc, M, N, Kp, alpha, beta, mirror, kstart_row, b_lower, st.s);
    ADMM_HIP_CHECK(hipGetLastError());
    std::vector<T> after(before.size());
    ADMM_HIP_CHECK(hipMemcpyAsync(after.data(), out, after.size() * sizeof(T), hipMemcpyDeviceToHost, st.s));
    st.sync();
    long long touched = 0, first_row = -1, first_col = -1;
    for (int j = 0; j < ccols; ++j)
        for (long long i = (j < N ? M : 0); i < ldc; ++i)
            if (std::memcmp(&after[(size_t)j * ldc + i], &before[(size_t)j * ldc + i], sizeof(T)) != 0 && touched++ == 0) { first_row = i; first_col = j; }
    for (int j = 0; j < N; ++j) std::memcpy(C + (size_t)j * M, &after[(size_t)j * ldc], (size_t)M * sizeof(T));
    if (touched != 0)
        throw Error(ADMM_ERR_INTERNAL, "gemm_nt wrote outside its " + std::to_string(M) + " x " + std::to_string(N) + " output: " + std::to_string(touched) +
                                           " entries of the padded storage changed, the first at (" + std::to_string(first_row) + ", " + std::to_string(first_col) + ")");
}
template void test_gemm_nt<float>(bool, bool, bool, bool, bool, int, int, int, double, double, const float*, const float*, float*);
template void test_gemm_nt<double>(bool, bool, bool, bool, bool, int, int, int, double, double, const double*, const double*, double*);

}  // namespace admm
