// Tall (n > p) Lasso / Elastic-net lambda path, device resident.
//
// Replaces, for n > p:  ADMMLassoTall / ADMMEnetTall driven by FADMMBase::solve
//   /root/reference/src/FADMMBase.h:185-265, ADMMLassoTall.h:55-231, ADMMEnet.h:19-58,
//   and the lambda loop of Lasso.cpp:97-124.
//
// Design (MI355X-first, not a translation):
//  * rho is fixed along the whole path (ADMMLassoTall.h:97, init only at i == 0), so the
//    Cholesky solve of (X'X + rho I) is replaced by ONE cached symmetric inverse Minv (p x p
//    fp32, 4p^2 bytes) and the x-update becomes a bandwidth-bound dense mat-vec.
//  * Goldstein acceleration/restart makes the right-hand side depend on a decision taken from
//    global norms (FADMMBase.h:243-256), but only between TWO vectors that are both known one
//    iteration earlier: the momentum ratio (a-1)/a' follows from the previous a alone, so
//        u = fl(fl(X'y - adj_y) + rho adj_z)  with adj = (1+ratio) new - ratio old     ("accelerate")
//        w = fl(fl(X'y - y_old) + rho z_old)                                          ("restart": adj = old)
//    are formed by the tail of the previous iteration exactly as ADMMLassoTall.h:70-80 rounds them.
//    Two launches per ADMM iteration, no host round trip, no grid barrier, no atomics between them: the x-update streams Minv
//    ONCE, the tail does everything else.  The scalar decision (norm reduction, convergence, acceleration / restart, lambda
//    schedule) turns on ctl[par] and the norm partials P[par] alone, both written by EARLIER launches, so it is taken inside the
//    x-update launch, and (round 8, SYMV_VERDICT=3, the default) by every workgroup of it for itself:
//      - block 0, ONE EXTRA WORKGROUP beside the streaming ones, evaluates the rule and publishes what follows from it (tall_decide:
//        eps, a_next / tau_next, the lambda schedule, niter[], the trace, ctl[par ^ 1]) for the tail;
//      - every tile evaluates the same rule in its prologue (TallGate -> tall_norms_sum + tall_outcome, the functions block 0 calls,
//        on the same inputs in the same order), in the round trip of its tile descriptor, and knows before its first FMA whether it
//        multiplies u (accelerate, cold start) or w (restart) -- symv1_lower_kernel, one plane of partials, half the partial
//        stores, a tail with 16 loads per lane -- or that nobody will read this launch's products (once per converged lambda, and
//        the last decision of a path): then it leaves at once.  No workgroup reads what another workgroup of its launch writes.
//    Levels 0 - 2 of SYMV_VERDICT, and the sharded / refined paths, keep the earlier form: a = Minv u and b = Minv w from one stream
//    against the pair (symv2_lower_kernel), the tail picks x = a or x = b, and the decision, taken BESIDE the stream by block 0 only,
//    reaches the tiles of a discarded launch as a VERDICT word (symv_kernels.h: SymvVerdict) that late starters and running tiles
//    (between two 8-column chunks) may or may not see in time (profiles/r07_tall_dead_work.md: 89.1-90.7 ms per C2 path before,
//    85.8-87.8 with it).  profiles/tall_decide_first.md has the measurements of the default against that form.
//    (An earlier version used x = Minv u' + tau Minv w' with u' = X'y - y + rho z: equal in exact
//    arithmetic, but it bypasses the float rounding of the right-hand side, and with it the dead
//    band that lets the reference's stopping rule fire when rho * ulp(z) exceeds eps_dual -- tiny
//    lambda, unstandardised data.  tests/tools/fuzz_parity.py found paths running to maxit.)
//  * Minv is symmetric: for p >= 2048 the x-update reads only its lower triangle (symv_kernels.h,
//    2p^2 bytes); small problems use the full-matrix gemv_t (fewer, larger workgroups).
//  * Convergence test, acceleration scalars, the lambda schedule (init_warm), niter[] and the
//    beta snapshot all live on the device; the host only enqueues iteration batches and polls
//    a `done` word asynchronously.
//  * After a converged lambda the reference re-solves with an unchanged right-hand side
//    (adj_z/adj_y are not updated on the exit iteration, FADMMBase.h:237-238), so the first
//    x of the next lambda equals the last x: `mode == 0` reuses it instead of a mat-vec.
#include "prep.h"
#include "gemv_kernels.h"
#include "symv_kernels.h"
#include "solvers.h"
#include "sgl_host.h"
#include "box_host.h"
#include "comm.h"
#include "loop_driver.h"
#include "plan_host.h"
#include "peer_device.h"
#include "probe.h"

namespace admm {

struct TallCtl {
    double rho, lam, eps_primal, eps_dual, adj_a, adj_c, tau;
    double a_next, tau_next;   // a' and ratio (a - 1) / a' the NEXT decision uses if it accelerates (computed once, here)
    int mode;       // 1: x = a (accelerate) or b (restart), adj from (cur, old);  0: keep stored x / adj (first iteration after convergence)
    int restart;    // with mode 1: adj = old exactly
    int iter;       // index i of the iteration this block describes
    int lam_idx;
    int done;
    int first;
    int total;
    int fin_idx;    // >= 0: the lambda that finished at this decision (snapshot z, record niter)
    int fin_niter;
    int pad;
};

struct TallParams {
    int p, nwg, nseg, maxit, nlam, enet;
    long long part_stride;
    double eps_abs, eps_rel, alpha, sqrt_p;
    const double* lambdas;      // device, nlam values already rounded to float
    const float* XY;
    const float* a_part; const float* b_part;            // gemv_t partials [nseg][part_stride]   (full-matrix x-update)
    const float* dot0; const float* dot1; const float* axp0; const float* axp1;   // symv partials (lower-triangle x-update)
    long long ldo; int nrb, p32; SymvSched sched;
    float* x; float* z0; float* z1; float* y0; float* y1; float* adj_z; float* adj_y; float* u; float* w;
    TallCtl* ctl;               // [2]
    double* P;                  // [2][nwg][8] norm partials of the tails' workgroups; behind them a compact copy of columns 0 .. 2 (r^2, dz^2, daz^2),
                                // [2][3][nwg]: the same numbers, laid out so that 256 threads read a column as consecutive doubles (TallGate)
    float* beta;                // [nlam][p] snapshots of z (standardised scale)
    int* niter;                 // [nlam]
    int* done_host;             // pinned host word set when the path has finished (loop_driver.h: PinnedFlag)
#ifdef ADMM_HIP_PROBE
    long long* probe;           // dev build only (probe.h)
#endif
    double* trace;              // optional [trace_cap][kTraceFields] decision records (admm_hip_lasso_plan_trace_*), or NULL
    long long trace_cap;
    const float* refine_ab;     // refined x-update (ADMM_HIP_REFINE=1): the first solve's a | b (leading dimension refine_ld), to which the tail adds
    long long refine_ld;        // the correction it sums from the partials; NULL otherwise
    float* state;               // optional [state_cap][5][p] iterates x, z, y, adj_z, adj_y of every iteration (admm_hip_lasso_plan_state_*), or NULL
    long long state_cap;
    unsigned long long* verdict;     // the x-update's verdict words (symv_kernels.h: SymvVerdict), published by the decision; NULL where no tile reads them
    unsigned long long* early;       // counts of the tiles that left early in this run (behind the verdict words: kSyEarlySlots counters on lines of their own), or NULL
    unsigned long long run_tag;      // number of this run() of the plan, above the bits of `total` and the discard bit
};

// The verdict word of the decision that leaves `total` decisions taken: bit 0 = the products of the launch it rides on are not used.
__host__ __device__ inline unsigned long long tall_verdict_word(unsigned long long run_tag, int total, bool discard) {
    return run_tag | ((unsigned long long)(unsigned)total << 1) | (discard ? 1ull : 0ull);
}
constexpr int kVerdictShift = 33;                                              // run_tag = run number << 33
constexpr int kVerdictWords = kSyVerdictReplicas * kSyVerdictStride;           // the early-exit counter sits behind the copies, on a line of its own

constexpr int kTailThreads = 256;
constexpr int kGateCols = 3;              // columns of the norm partials a tile's gate needs: r^2, dz^2, daz^2 (compact copy behind P)
// P[par] as block 0 reads it (a 64-byte row per workgroup of the tail) and the compact copy of its first kGateCols columns
__host__ __device__ inline const double* tall_norm_rows(const double* P, int nwg, int par) { return P + (size_t)par * nwg * 8; }
__host__ __device__ inline size_t tall_norm_compact(int nwg, int par) { return (size_t)2 * nwg * 8 + (size_t)par * kGateCols * nwg; }
constexpr int kTailLanes = kSySumLanes;   // lanes cooperating on one element's partial sums
constexpr int kTailElems = kTailThreads / kTailLanes;

// Scalar control of one iteration, run by a single workgroup: reduce the previous iteration's norm
// partials, evaluate convergence / acceleration / restart / lambda schedule, publish ctl[par ^ 1].
// IN_LAUNCH: the norm partials were written (write-through) by other workgroups of the SAME launch (single-launch
// iteration below): they are read with agent-scope loads that bypass this XCD's L2.
__device__ __forceinline__ double tall_load_partial(const double* p, bool in_launch) {
    if (!in_launch) return *p;
    return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ void tall_store_wt(float* p, float v) {       // write-through store (visible to other XCDs without a fence)
    __hip_atomic_store(reinterpret_cast<unsigned int*>(p), __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void tall_store_wt(double* p, double v) {
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- The decision rule, one copy (round 8).  What a decision turns on -- three comparisons on ctl[par] and the sums of the norm partials
// P[par] -- was written by EARLIER launches, so any 256-thread workgroup of the x-update launch can evaluate it: block 0 (tall_decide
// below, which goes on to publish ctl[par ^ 1]) and, on the decide-first path (SYMV_VERDICT=3), every tile in its prologue (TallGate),
// which then knows before its first FMA which vector it multiplies, or that it need not run.  Same functions, same inputs, same order
// of every addition: the outcome a tile computes equals block 0's by construction, and no workgroup of a launch reads anything another
// workgroup of that launch writes -- no flag, no spin, no atomic wait, no fence.
enum { TALL_COLD = 0, TALL_CONVERGED = 1, TALL_ACCELERATE = 2, TALL_RESTART = 3 };
struct TallOutcome {
    int code;        // TALL_*
    int fin;         // the lambda of ctl[par] finishes at this decision (converged, or by maxit)
    int done;        // ... and it was the last one: the path is finished
    double rp, rd, c;
    // what the tiles of the launch that takes this decision do: nobody reads their products after a converged lambda (the tail keeps
    // the stored x) or at the end of the path; otherwise the tail takes x = b on a restart and x = a else (cold start included)
    __device__ __forceinline__ bool discard() const { return code == TALL_CONVERGED || done != 0; }
    __device__ __forceinline__ int pick() const { return code == TALL_RESTART ? 1 : 0; }
};

// Norm partials of P[par]: thread t sums rows t, t + 256, ... in that order, then block_sum.  Block 0 reads the 64-byte rows of P; the
// tiles read the compact copy the tails write beside it (tall_publish_norms) -- the same doubles, but a column is consecutive, so a wave's
// load touches 4 lines instead of 64: 1600 tiles asking for 157 strided lines each at the start of a launch cost the regular launches
// 2 us (measured: 34.2 against 32.2 us), the compact copy is 59 lines.  The first two rows of a thread (all of them
// up to p = 16384) are requested without a wait between them, so that a caller can issue other loads behind them (tall_norms_request);
// tall_norms_sum adds them in the loop's order and continues the loop.  NK: the first NK of the 6 columns (a tile needs r^2, dz^2, daz^2;
// the columns are summed independently, so NK = 3 returns the bits NK = 6 returns for them).
// (rs, cs): strides of a workgroup's row and of a column in Pin -- (8, 1) for the rows of P, (1, nwg) for the compact copy.
// Round 11: the requests are branch-free -- a thread without a row asks for the last row instead (nwg >= 1: always a valid address) and
// tall_norms_sum adds +0.0 in its place -- and nothing in tall_norms_request USES what it loads.  (Guarded by `w < nwg` on both sides,
// the load and its add were merged into one predicated block per column, the add -- and a wait for the load -- directly behind each
// request: three serialised round trips at the head of every tile.)  The bits are the guarded form's: a skipped add left acc = +0.0
// (first row) or 0.0 + v, which is never -0.0 (second row), and x + (+0.0) is x for either.
template <int NK> struct TallNormReq { double v[2][NK]; };
template <int NK, bool IN_LAUNCH>
__device__ __forceinline__ TallNormReq<NK> tall_norms_request(const double* Pin, int nwg, int rs, int cs) {
    TallNormReq<NK> r;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int w = min((int)threadIdx.x + j * kTailThreads, nwg - 1);
#pragma unroll
        for (int k = 0; k < NK; ++k) r.v[j][k] = tall_load_partial(Pin + (size_t)w * rs + (size_t)k * cs, IN_LAUNCH);
    }
    return r;
}
template <int NK, bool IN_LAUNCH>
__device__ __forceinline__ void tall_norms_sum(const TallNormReq<NK>& r, const double* Pin, int nwg, int rs, int cs, double (&acc)[NK], double* scratch) {
#pragma unroll
    for (int k = 0; k < NK; ++k) acc[k] = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const bool live = (int)threadIdx.x + j * kTailThreads < nwg;
#pragma unroll
        for (int k = 0; k < NK; ++k) acc[k] += live ? r.v[j][k] : 0.0;
    }
    for (int w = threadIdx.x + 2 * kTailThreads; w < nwg; w += kTailThreads) {
#pragma unroll
        for (int k = 0; k < NK; ++k) acc[k] += tall_load_partial(Pin + (size_t)w * rs + (size_t)k * cs, IN_LAUNCH);
    }
    block_sum<double, NK>(acc, scratch);
}

// The comparisons.  Contraction is off and the one fused product is written out (it is the form the compiler chose for this expression
// before the rule was shared): the two callers must not be left to round it differently.
__device__ __forceinline__ TallOutcome tall_outcome(const TallCtl& in, double r2, double dz2, double daz2, int maxit, int nlam) {
#pragma clang fp contract(off)
    TallOutcome o;
    o.code = TALL_COLD; o.fin = 0; o.done = 0; o.rp = 0; o.rd = 0; o.c = 0;
    if (in.first) return o;                            // cold start: adj = 0, x = Minv X'y
    const double rp = sqrt(r2);                        // resid_primal            FADMMBase.h:208
    const double rd = in.rho * sqrt(dz2);              // resid_dual              ADMMLassoTall.h:150-153
    o.rp = rp; o.rd = rd;
    if (rp < in.eps_primal && rd < in.eps_dual) {      // converged()             FADMMBase.h:213-217
        o.code = TALL_CONVERGED; o.fin = 1;
    } else {
        const double c = fma(in.rho * rp, rp, in.rho * daz2);      // compute_resid_combined  ADMMLassoTall.h:154-161
        o.c = c;
        o.code = c < 0.999 * in.adj_c ? TALL_ACCELERATE : TALL_RESTART;      // FADMMBase.h:243-256
        if (in.iter + 1 >= maxit) o.fin = 1;           // loop ran out: `return i + 1` with i == maxit
    }
    if (o.fin && in.lam_idx + 1 >= nlam) o.done = 1;
    return o;
}

// The gate of symv1_lower_kernel (symv_kernels.h): the decision of this launch, taken by every tile for itself.
struct TallGate {
    const TallCtl* ctl;       // &ctl[par]
    const double* Pin;        // the compact copy of P[par]: [kGateCols][nwg], the numbers block 0 reads from the rows of P[par]
    int nwg, maxit, nlam;
    struct Req { TallCtl in; TallNormReq<kGateCols> n; };
    __device__ __forceinline__ void pin() const { asm volatile("" :: "s"(ctl), "s"(Pin), "s"(nwg), "s"(maxit), "s"(nlam)); }
    __device__ __forceinline__ Req request() const {
        Req r;
        r.in = *ctl;
        r.n = tall_norms_request<kGateCols, false>(Pin, nwg, 1, nwg);
        return r;
    }
    __device__ __forceinline__ void sums(const Req& r, double* lds, double (&acc)[kGateCols]) const {
        tall_norms_sum<kGateCols, false>(r.n, Pin, nwg, 1, nwg, acc, lds);
    }
    __device__ __forceinline__ int decide(const Req& r, double* lds) const {
        if (r.in.done) return kSyGateLeave;            // (the kernel has returned on its `done` word already)
        double acc[kGateCols];
        sums(r, lds, acc);
        const TallOutcome o = tall_outcome(r.in, acc[0], acc[1], acc[2], maxit, nlam);
        return o.discard() ? kSyGateLeave : o.pick();
    }
};
static_assert(kSyThreads == kTailThreads, "the tiles and the deciding workgroup share the decision rule: one thread <-> partial mapping");
static_assert(kSyGateScratch >= 6 * (kTailThreads / 64), "block_sum's scratch");

// Block 0's part: the outcome applied -- eps of the next iteration, a_next / tau_next, the lambda schedule, niter[], the trace record,
// done_host and ctl[par ^ 1].
template <bool IN_LAUNCH = false>
__device__ void tall_decide(const TallParams& q, int par) {
    __shared__ double dscratch[6 * (kTailThreads / 64)];
    WIDE_PROBE_DECL
    WIDE_PROBE(0);
    const TallCtl in = q.ctl[par];
    TallCtl* outp = &q.ctl[par ^ 1];
    if (in.done) {
        if (threadIdx.x == 0) { TallCtl o = in; o.fin_idx = -1; *outp = o; }   // keep `done` sticky in both slots
        return;
    }
    WIDE_PROBE(1);
    double acc[6];
    const double* Pin = tall_norm_rows(q.P, q.nwg, par);
    tall_norms_sum<6, IN_LAUNCH>(tall_norms_request<6, IN_LAUNCH>(Pin, q.nwg, 8, 1), Pin, q.nwg, 8, 1, acc, dscratch);
    if (threadIdx.x != 0) return;
    WIDE_PROBE(2);
    const double x2 = acc[3], z2 = acc[4], y2 = acc[5];
    const TallOutcome oc = tall_outcome(in, acc[0], acc[1], acc[2], q.maxit, q.nlam);
    const double tr_rp = oc.rp, tr_rd = oc.rd, tr_c = oc.c;
    double tr_code = ADMM_TRACE_COLD;
    TallCtl out = in;
    out.first = 0;
    out.fin_idx = -1; out.fin_niter = 0;
    if (oc.code == TALL_COLD) {
        out.mode = 1; out.tau = 0.0; out.restart = 0;  // cold start: adj = 0, x = Minv X'y
    } else {
        if (oc.code == TALL_CONVERGED) {
            out.fin_idx = in.lam_idx; out.fin_niter = in.iter + 1;
            out.mode = 0;
            tr_code = ADMM_TRACE_CONVERGED;
        } else {
            const double old_c = in.adj_c;
            if (oc.code == TALL_ACCELERATE) {          // FADMMBase.h:243-249
                out.adj_a = in.a_next; out.adj_c = oc.c; out.tau = in.tau_next; out.restart = 0;
                tr_code = ADMM_TRACE_ACCELERATE;
            } else {                                   // restart                 FADMMBase.h:250-256
                out.adj_a = 1.0; out.adj_c = old_c / 0.999; out.tau = -1.0; out.restart = 1;
                tr_code = ADMM_TRACE_RESTART;
            }
            out.mode = 1;
            out.iter = in.iter + 1;
            if (oc.fin) {                              // loop ran out: `return i + 1` with i == maxit
                out.fin_idx = in.lam_idx; out.fin_niter = q.maxit + 1;
            }
        }
        if (out.fin_idx >= 0) {                        // next lambda: init_warm keeps x,z,y,adj,a,c,rho (ADMMLassoTall.h:219-230)
            out.lam_idx = in.lam_idx + 1;
            out.iter = 0;
            if (oc.done) out.done = 1;
            else out.lam = q.lambdas[out.lam_idx];
            q.niter[out.fin_idx] = out.fin_niter;
        }
    }
    // Verdict-word path (SYMV_VERDICT=1|2; q.verdict is NULL on the decide-first path, whose tiles know for themselves): the tiles of THIS
    // launch compute products the tail will not read when the decision is "keep the stored x" or "finished": tell the ones that have not
    // started yet, as early as it is known (symv_kernels.h: SymvVerdict).  Only a discard is ever published -- any other word, a missing
    // one included, means "stream".  Write-through, no fence: one word, nothing else to be seen with it.
    if (q.verdict != nullptr && oc.discard()) {
        const unsigned long long word = tall_verdict_word(q.run_tag, in.total + 1, true);
        for (int r = 0; r < kSyVerdictReplicas; ++r)
            __hip_atomic_store(q.verdict + (size_t)r * kSyVerdictStride, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // eps for the iteration about to run, from the CURRENT iterate (FADMMBase.h:187-188, ADMMLassoTall.h:141-149)
    out.eps_primal = fmax(sqrt(x2), sqrt(z2)) * q.eps_rel + q.sqrt_p * q.eps_abs;
    out.eps_dual = sqrt(y2) * q.eps_rel + q.sqrt_p * q.eps_abs;
    out.a_next = 0.5 + 0.5 * sqrt(1.0 + 4.0 * out.adj_a * out.adj_a);
    out.tau_next = (out.adj_a - 1.0) / out.a_next;
    out.total = in.total + 1;
    *outp = out;
    if (out.done) *q.done_host = 1;
    WIDE_PROBE(3);
    WIDE_PROBE_FLUSH(2, in.total);
    if (q.trace != nullptr && in.total < q.trace_cap) {      // what FADMMBase.h:135-170 (print_row, commented out there) would print
        double* t = q.trace + (size_t)in.total * ADMM_TRACE_FIELDS;
        t[0] = in.lam_idx; t[1] = in.iter; t[2] = in.eps_primal; t[3] = in.eps_dual; t[4] = tr_rp; t[5] = tr_rd;
        t[6] = tr_c; t[7] = in.adj_c; t[8] = tr_code; t[9] = in.rho; t[10] = in.rho; t[11] = in.lam;
    }
}

struct TallDecideExtra {
    static constexpr bool kHas = true;
    TallParams q; int par;
    __device__ void operator()() const { tall_decide<false>(q, par); }
};

// (1 + ratio) * cur - ratio * old without contraction, like the reference build (FADMMBase.h:247-248): the
// same value is formed twice, as the candidate right-hand side and as adj of the next iteration.
__device__ __forceinline__ float tall_extrapolate(float t1, float t, float cur, float old) {
    // plain operators under contract(off): HIP's __fmul_rn / __fsub_rn are inline `x * y` / `x - y` written in a header that is
    // compiled with contraction allowed, and the two were fused into v_pk_fma_f32 all the same
#pragma clang fp contract(off)
    const float a = t1 * cur;
    const float b = t * old;
    return a - b;
}

// State of one coordinate and its update: everything after the x-update in one iteration
// (next_z, residual, dual update, norms, right-hand sides of the next x-update).
struct TallElem { float zc, yc, zo, yo, adjz, adjy, x, xy; };

__device__ __forceinline__ TallElem tall_load_elem(const TallParams& q, int par, int i) {
    const float* zc_ = par ? q.z1 : q.z0; const float* yc_ = par ? q.y1 : q.y0;
    const float* zo_ = par ? q.z0 : q.z1; const float* yo_ = par ? q.y0 : q.y1;
    TallElem e;
    e.zc = zc_[i]; e.yc = yc_[i]; e.zo = zo_[i]; e.yo = yo_[i]; e.adjz = q.adj_z[i]; e.adjy = q.adj_y[i]; e.x = q.x[i]; e.xy = q.XY[i];
    return e;
}

// soft_threshold of the Lasso: the compare in double, the result rounded once (ADMMLassoTall.h:55-69)
__device__ __forceinline__ float tall_soft(float vec, double pen) {
    const double v = (double)vec;
    return v > pen ? (float)(v - pen) : (v < -pen ? (float)(v + pen) : 0.f);
}

// block soft-threshold of a group / row of squared norm nrm2: the factor max(0, 1 - pen / ||v||)
__device__ __forceinline__ double tall_block_shrink(double nrm2, double pen) {
    const double nrm = sqrt(nrm2);
    return nrm > pen ? 1.0 - pen / nrm : 0.0;
}

template <bool WT = false>      // WT: u, w are consumed by other workgroups of the same launch -> write-through stores
__device__ __forceinline__ void tall_update_elem(const TallParams& q, const TallCtl& c, int par, int i, const TallElem& e, float a, float b, double (&acc)[6]) {
    // The reference is built without fused multiply-adds (R's default flags on x86-64: no -march, /root/reference/src/Makevars):
    // every product below rounds before it is added, as there.  (__fmul_rn / __fadd_rn are plain operators in HIP and were
    // contracted all the same: found by the stepwise check of oracle/stepcheck.py, round 3.)
#pragma clang fp contract(off)
    float* zo_ = par ? q.z0 : q.z1; float* yo_ = par ? q.y0 : q.y1;
    const float zc = e.zc, yc = e.yc, zo = e.zo, yo = e.yo;
    if (c.fin_idx >= 0) q.beta[(size_t)c.fin_idx * q.p + i] = zc;     // get_z() snapshot (Lasso.cpp:108)
    if (c.done) return;
    float adjz, adjy, x;
    if (c.mode) {
        if (c.restart) { adjz = zo; adjy = yo; x = b; }
        else {
            const float t = (float)c.tau, t1 = (float)(1.0 + c.tau);
            adjz = tall_extrapolate(t1, t, zc, zo);       // (1 + ratio) * aux_z - ratio * old_z   FADMMBase.h:247-248
            adjy = tall_extrapolate(t1, t, yc, yo);
            x = a;
        }
    } else { adjz = e.adjz; adjy = e.adjy; x = e.x; }
    const float rho_f = (float)c.rho;
    const float vec = x + adjy / rho_f;        // next_z: main_x + adj_y / rho            ADMMLassoTall.h:83
    const double pen = c.lam / c.rho;
    float zn;
    if (!q.enet) zn = tall_soft(vec, pen);
    else {                                   // enet()                                  ADMMEnet.h:24-40
        const float thresh = (float)(q.alpha * pen);
        const float denom = (float)(1.0 + pen * (1.0 - q.alpha));
        zn = vec > thresh ? (vec - thresh) / denom : (vec < -thresh ? (vec + thresh) / denom : 0.f);
    }
    const float r = x - zn;                    // next_residual                            ADMMLassoTall.h:86-95
    const float yn = adjy + rho_f * r;         // dual_y = adj_y + rho * newr              FADMMBase.h:210
    const float dz = zn - zc, daz = zn - adjz;
    acc[0] = (double)r * r; acc[1] = (double)dz * dz; acc[2] = (double)daz * daz;
    acc[3] = (double)x * x; acc[4] = (double)zn * zn; acc[5] = (double)yn * yn;
    q.x[i] = x; zo_[i] = zn; yo_[i] = yn; q.adj_z[i] = adjz; q.adj_y[i] = adjy;
    if (q.state != nullptr && c.total < q.state_cap) {     // record c.total = the trace record that will judge this iteration
        float* s = q.state + (size_t)c.total * 5 * q.p;
        s[i] = x; s[q.p + i] = zn; s[2 * (size_t)q.p + i] = yn; s[3 * (size_t)q.p + i] = adjz; s[4 * (size_t)q.p + i] = adjy;
    }
    // both possible right-hand sides of the next x-update, rounded as ADMMLassoTall.h:70-80 does
    const float tn = (float)c.tau_next, tn1 = (float)(1.0 + c.tau_next);
    const float adjz_a = tall_extrapolate(tn1, tn, zn, zc), adjy_a = tall_extrapolate(tn1, tn, yn, yc);
    const float un = (float)((double)(e.xy - adjy_a) + c.rho * (double)adjz_a);
    const float wn = (float)((double)(e.xy - yc) + c.rho * (double)zc);
    if (WT) { tall_store_wt(q.u + i, un); tall_store_wt(q.w + i, wn); }
    else { q.u[i] = un; q.w[i] = wn; }
}

// Block sum of the six norms into P[par ^ 1][blockIdx.x]; every thread of the workgroup calls it.  Only the owner lanes (sub == 0)
// hold values, so wave_sum's xor-4 / 2 / 1 steps would add exact zeros: the top half of the halving butterfly (xor 32 / 16 / 8)
// leaves the wave total of value k in lane 8 k, bit-identical to block_sum<double, 6> at 7 exchanges instead of 36.
__device__ __forceinline__ void tall_publish_norms(const TallParams& q, int par, const double (&acc)[6], double* scratch) {
    static_assert(kTailLanes == 8, "owner lanes are the multiples of 8");
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const double v8[8] = {acc[0], acc[1], acc[2], acc[3], acc[4], acc[5], 0.0, 0.0};
    const double tot = halving_sum8_top(v8, lane);
    if ((lane & 7) == 0 && lane < 48) scratch[(lane >> 3) * (kTailThreads / 64) + wid] = tot;
    __syncthreads();
    if (threadIdx.x < 6) {
        double sum = 0;
        for (int ww = 0; ww < kTailThreads / 64; ++ww) sum += scratch[threadIdx.x * (kTailThreads / 64) + ww];
        q.P[((size_t)(par ^ 1) * q.nwg + blockIdx.x) * 8 + threadIdx.x] = sum;
        if (threadIdx.x < kGateCols) q.P[tall_norm_compact(q.nwg, par ^ 1) + (size_t)threadIdx.x * q.nwg + blockIdx.x] = sum;
    }
}

// Element-wise part of one iteration.  `c` = the control block published by this iteration's decision.
// MODE 0: x-update results as gemv_t partial rows; 1: as the symmetric mat-vec's partial arrays; 2: row-sharded over the
// PEER exchange -- wait for the K flags, then sum the K ranks' shares straight out of the exchange slots; 4 (TAIL_SYMV1): the
// decide-first x-update (symv1_lower_kernel) left ONE plane of partials, those of the vector this iteration's decision picked.
enum { TAIL_GEMV = 0, TAIL_SYMV = 1, TAIL_PEER = 2, TAIL_PEER1 = 3, TAIL_SYMV1 = 4 };

// The kTailLanes lanes of one element add up what each of them summed.
__device__ __forceinline__ void tall_lane_sum(float& a, float& b) {
#pragma unroll
    for (int m = 1; m < kTailLanes; m <<= 1) { a += __shfl_xor(a, m, 64); b += __shfl_xor(b, m, 64); }
}

// x-update results a = Minv u, b = Minv w of element i (single device): kTailLanes lanes share one element and issue all their partial
// loads at once, then combine with shuffles.  Nothing here depends on the control block.
// `behind`: the caller's own loads of the coordinate (only lanes with valid == true may have any).  TAIL_SYMV1 issues them behind its
// sixteen partial requests and ahead of their first use (symv_kernels.h: symv_sum_partials1), the other forms ahead of the partials as before.
template <int MODE, typename Behind = SymvNothingBehind>
__device__ __forceinline__ void tall_gather_ab(const TallParams& q, int i, int sub, bool valid, float& a, float& b, Behind behind = Behind()) {
    if (MODE != TAIL_SYMV1) behind();
    if (MODE == TAIL_SYMV) {
        symv_sum_partials<kTailLanes>(q.dot0, q.dot1, q.axp0, q.axp1, q.ldo, q.nrb, q.sched, q.p32, i, sub, valid, a, b);
        return;
    }
    if (MODE == TAIL_SYMV1) {
        // Plane 0 holds Minv u if the decision was "accelerate" and Minv w if it was "restart": the one the tail reads.  Returned as both,
        // so that `x = restart ? b : a` (tall_update_elem and its restatements) picks it either way -- and no load depends on ctl.
        a = b = symv_sum_partials1<kTailLanes>(q.dot0, q.axp0, q.ldo, q.nrb, q.sched, q.p32, i, sub, valid, behind);
        return;
    }
    a = 0.f; b = 0.f;
    if (valid) {
        for (int k = sub; k < q.nseg; k += kTailLanes) {
            const size_t o = (size_t)k * q.part_stride + i;
            a += q.a_part[o]; b += q.b_part[o];
        }
    }
    tall_lane_sum(a, b);
}

// TAIL_PEER1: producer and consumer of the exchange in ONE launch -- every workgroup sums its elements of this rank's share,
// writes them into every rank's slot and counts itself in (the last one raises the flags), then waits for the K flags like
// TAIL_PEER.  A workgroup waits for flags that need ALL workgroups of this launch (on every rank) to have published, so
// the launch must be resident as a whole; the host only chooses it when the grid is at most half of what the device holds.
template <int MODE>
__global__ void __launch_bounds__(kTailThreads)
tall_tail_kernel(TallParams q, int par, PeerExchange ex) {
    __shared__ double scratch[6 * (kTailThreads / 64)];
    WIDE_PROBE_DECL
    WIDE_PROBE(0);
    const TallCtl c = q.ctl[par ^ 1];
    // Every load below is independent of `c` (the ping-pong parity equals the launch parity because
    // the decision advances `total` once per launch), so the whole kernel is one memory round trip -- for TAIL_SYMV1 also as compiled:
    // the sixteen partial requests go first and the owner lane's eight loads behind them, ahead of any wait (tall_gather_ab's `behind`).
    const int sub = threadIdx.x & (kTailLanes - 1);
    const int i = blockIdx.x * kTailElems + threadIdx.x / kTailLanes;
    const bool valid = i < q.p;
    const bool owner = valid && sub == 0;
    TallElem e = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const auto load_elem = [&]() { if (owner) e = tall_load_elem(q, par, i); };      // the owner lane's eight loads; tall_gather_ab places them
    float a = 0.f, b = 0.f;
    if (MODE == TAIL_PEER || MODE == TAIL_PEER1) {
        load_elem();
        const bool live = !q.ctl[par].done;                          // finished in an earlier launch: nothing pushed, nothing to wait for (replicated flag: all ranks agree)
        if (MODE == TAIL_PEER1 && live) {
            float sa, sb;
            symv_sum_partials<kTailLanes>(q.dot0, q.dot1, q.axp0, q.axp1, q.ldo, q.nrb, q.sched, q.p32, i, sub, valid, sa, sb);
            if (valid) {
                for (int dst = sub; dst < ex.nranks; dst += kTailLanes)
                    peer_store_f32x2(reinterpret_cast<float*>(peer_dst_slot(ex, dst)) + 2 * (size_t)i, sa, sb);
            }
            peer_publish(ex, gridDim.x);
        }
        // the producing launch (or the block above) pushed unless the solve was already finished
        const bool ok = live ? peer_wait_relaxed(ex) : false;
        if (ok && valid) {
            for (int r = sub; r < ex.nranks; r += kTailLanes) {          // rank order fixed by the lane pattern: identical on every rank
                const float2 v = peer_load_f32x2(reinterpret_cast<const float*>(peer_src_slot(ex, r)) + 2 * (size_t)i);    // (a_i, b_i) interleaved
                a += v.x; b += v.y;
            }
        }
        tall_lane_sum(a, b);
    } else {
        tall_gather_ab<MODE>(q, i, sub, valid, a, b, load_elem);
        if (MODE == TAIL_SYMV && q.refine_ab != nullptr && valid) {      // x = x1 + Minv (rhs - M x1): the partials hold the correction
            a = q.refine_ab[i] + a;
            b = q.refine_ab[q.refine_ld + i] + b;
        }
    }
    if (c.done && c.fin_idx < 0) return;
    WIDE_PROBE(1);

    double acc[6] = {0, 0, 0, 0, 0, 0};
    if (owner) tall_update_elem(q, c, par, i, e, a, b, acc);
    if (c.done) return;
    WIDE_PROBE(2);
    tall_publish_norms(q, par, acc, scratch);
    WIDE_PROBE(3);
    WIDE_PROBE_FLUSH(blockIdx.x == 0 ? 0 : (blockIdx.x == gridDim.x - 1 ? 1 : -1), c.total - 1);
}

// ---- group lasso (admm_hip_grplasso): the same iteration with a block soft-threshold as next_z
//     z_g = v_g max(0, 1 - pen_g / ||v_g||_2),  v = x + adj_y / rho,  pen_g = lambda w_g / rho
// A coordinate needs the norm of its whole group before it can be written, which tall_tail_kernel (one owner lane per coordinate,
// no coordinate sees another) cannot express.  This tail does everything that one does for its coordinates plus the norms, in the
// same launch: the host packs whole groups into TILES -- a run of consecutive groups of at most kTailElems coordinates in all,
// one workgroup, one pass; a group larger than that gets a workgroup of its own, which walks it in passes of kTailElems -- and the
// coordinates' v go through LDS.  Norms are sums of (double) v^2 in a fixed order: no atomics, the same bits from run to run.
// Shared with that tail as functions: tall_gather_ab, tall_soft, tall_publish_norms (and tall_block_shrink with the multi-task tail).
// The choice of (adj_z, adj_y, x) and the second half restate tall_update_elem and must be kept equal to it by hand: called as shared
// functions they cost the 1024-column group and the multi-task tail 0.3 - 1.5 % of an iteration (profiles/tall_tail_shared.md).
// A group of ONE column takes tall_soft, so singleton groups of weight 1 reproduce admm_hip_lasso exactly (the tiles are then
// tall_tail_kernel's workgroups, the norm partials P the same sums).
//
// SPARSE (admm_hip_sgl): the prox of lambda (alpha sum_j u_j |b_j| + (1 - alpha) sum_g w_g ||b_g||_2) is the element-wise soft-threshold
// followed by the block one, so a group of several columns stores  s_j = tall_soft(v_j, lambda l1_j / rho)  where the plain form
// stores v_j, and everything after the first half -- the norm, the shrink, the six norm partials, the next right-hand sides -- is the
// same code on s.  The owner lane loads l1_j (sgl_host.h: alpha u_j; alpha never reaches the device)
// beside the coordinate's other loads: its address needs neither `c` nor more of the tile entry than those do, so the kernel is still
// one memory round trip per pass.  A one-column group keeps v and takes the scalar threshold with GroupCoord.w = l1_j + wg_g.
struct GroupCoord { int gs, gn; double w; };      // per coordinate: first column, size and weight of its group
struct GroupTailParams {
    const int2* tiles;                            // [TallParams.nwg]  (first coordinate, number of coordinates)
    const GroupCoord* coord;                      // [p]
    const double* l1;                             // [p] element-wise threshold weights (SPARSE only; NULL otherwise)
};
constexpr int kGroupMax = ADMM_HIP_GROUP_MAX;

template <int MODE, bool SPARSE = false>
__global__ void __launch_bounds__(kTailThreads)
tall_group_tail_kernel(TallParams q, int par, GroupTailParams gp) {
#pragma clang fp contract(off)
    static_assert(MODE == TAIL_GEMV || MODE == TAIL_SYMV || MODE == TAIL_SYMV1, "single device");
    __shared__ double scratch[6 * (kTailThreads / 64)];
    __shared__ double snrm[kTailElems];
    // the tile's coordinates between the two halves of the update: x, adj_z, adj_y, v and what the second half still needs of the loads
    __shared__ float sx[kGroupMax], sadjz[kGroupMax], sadjy[kGroupMax], sv[kGroupMax], szc[kGroupMax], syc[kGroupMax], sxy[kGroupMax];
    const TallCtl c = q.ctl[par ^ 1];
    const int2 tile = gp.tiles[blockIdx.x];
    const int i0 = tile.x, cnt = tile.y;
    const int sub = threadIdx.x & (kTailLanes - 1), e = threadIdx.x / kTailLanes;
    const int npass = (cnt + kTailElems - 1) / kTailElems;
    const bool big = cnt > kTailElems;                                   // one group walked in passes; otherwise whole small groups, one pass
    const GroupCoord gc = gp.coord[i0 + min(e, cnt - 1)];                // (big: every coordinate of the tile has the same)
    float* zo_ = par ? q.z0 : q.z1; float* yo_ = par ? q.y0 : q.y1;
    const float rho_f = (float)c.rho;

    // ---- first half: x-update results, extrapolation, v = x + adj_y / rho
    for (int k = 0; k < npass; ++k) {
        const int s = k * kTailElems + e, i = i0 + s;
        const bool valid = s < cnt, owner = valid && sub == 0;
        TallElem el = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (owner) el = tall_load_elem(q, par, i);
        double l1 = 0.0;
        if (SPARSE && owner) l1 = gp.l1[i];
        float a, b;
        tall_gather_ab<MODE>(q, i, sub, valid, a, b);
        if (c.done && c.fin_idx < 0) return;
        if (owner) {
            if (c.fin_idx >= 0) q.beta[(size_t)c.fin_idx * q.p + i] = el.zc;     // get_z() snapshot (Lasso.cpp:108)
            if (!c.done) {
                float adjz, adjy, x;
                if (c.mode) {
                    if (c.restart) { adjz = el.zo; adjy = el.yo; x = b; }
                    else {
                        const float t = (float)c.tau, t1 = (float)(1.0 + c.tau);
                        adjz = tall_extrapolate(t1, t, el.zc, el.zo);
                        adjy = tall_extrapolate(t1, t, el.yc, el.yo);
                        x = a;
                    }
                } else { adjz = el.adjz; adjy = el.adjy; x = el.x; }
                float vec = x + adjy / rho_f;
                if (SPARSE && gc.gn > 1) vec = tall_soft(vec, c.lam * l1 / c.rho);      // s = soft(v, lambda l1 / rho)
                sx[s] = x; sadjz[s] = adjz; sadjy[s] = adjy; sv[s] = vec;
                szc[s] = el.zc; syc[s] = el.yc; sxy[s] = el.xy;
            }
        }
    }
    if (c.done) return;
    __syncthreads();

    // ---- squared norm of this lane's group (SPARSE: of s), in double, in a fixed order
    double nrm2 = 0.0;
    if (big) {
        if (sub == 0) {
            double part = 0.0;
            for (int s = e; s < cnt; s += kTailElems) { const double v = (double)sv[s]; part += v * v; }
            snrm[e] = part;
        }
        __syncthreads();
        for (int m = 0; m < kTailElems; ++m) nrm2 += snrm[m];
    } else if (sub == 0 && e < cnt && gc.gn > 1) {
        const int s0 = gc.gs - i0;
        for (int m = 0; m < gc.gn; ++m) { const double v = (double)sv[s0 + m]; nrm2 += v * v; }
    }
    const double pen = c.lam * gc.w / c.rho;
    double shrink = 0.0;                                                // max(0, 1 - pen / ||v_g||)
    if (gc.gn > 1) shrink = tall_block_shrink(nrm2, pen);

    // ---- second half: next_z, residual, dual update, norms, the right-hand sides of the next x-update (tall_update_elem's, restated)
    double acc[6] = {0, 0, 0, 0, 0, 0};
    const float tn = (float)c.tau_next, tn1 = (float)(1.0 + c.tau_next);
    for (int k = 0; k < npass; ++k) {
        const int s = k * kTailElems + e, i = i0 + s;
        if (!(s < cnt && sub == 0)) continue;
        const float x = sx[s], adjz = sadjz[s], adjy = sadjy[s], vec = sv[s], zc = szc[s], yc = syc[s], xy = sxy[s];
        const double v = (double)vec;
        float zn;
        if (gc.gn == 1) zn = tall_soft(vec, pen);
        else zn = (float)(v * shrink);
        const float r = x - zn;
        const float yn = adjy + rho_f * r;
        const float dz = zn - zc, daz = zn - adjz;
        acc[0] += (double)r * r; acc[1] += (double)dz * dz; acc[2] += (double)daz * daz;
        acc[3] += (double)x * x; acc[4] += (double)zn * zn; acc[5] += (double)yn * yn;
        q.x[i] = x; zo_[i] = zn; yo_[i] = yn; q.adj_z[i] = adjz; q.adj_y[i] = adjy;
        if (q.state != nullptr && c.total < q.state_cap) {
            float* st = q.state + (size_t)c.total * 5 * q.p;
            st[i] = x; st[q.p + i] = zn; st[2 * (size_t)q.p + i] = yn; st[3 * (size_t)q.p + i] = adjz; st[4 * (size_t)q.p + i] = adjy;
        }
        const float adjz_a = tall_extrapolate(tn1, tn, zn, zc), adjy_a = tall_extrapolate(tn1, tn, yn, yc);
        q.u[i] = (float)((double)(xy - adjy_a) + c.rho * (double)adjz_a);
        q.w[i] = (float)((double)(xy - yc) + c.rho * (double)zc);
    }
    tall_publish_norms(q, par, acc, scratch);
}

// ---- box-constrained, weighted elastic net (admm_hip_boxenet): the same iteration with a per-coordinate penalty and a clamp as next_z
//     z_j = clamp(prox_j(v_j), lo_j, hi_j),  v = x + adj_y / rho,  pen_j = lambda u_j / rho  (this order: u_j = 1 gives lambda / rho exactly)
//     Lasso prox (TallParams.enet == 0):  tall_soft(v_j, pen_j)
//     elastic net:  thresh = (float)(alpha pen_j), denom = (float)(1 + pen_j (1 - alpha)), (v_j -+ thresh) / denom beyond the threshold, else 0
// The prox of lambda u_j (alpha |z| + (1 - alpha) z^2 / 2) plus the indicator of [lo_j, hi_j], lo_j <= 0 <= hi_j, is a convex problem
// in one variable: its minimiser is the unconstrained one moved to the nearest point of the interval, so the clamp makes the prox
// exact and there is no inner iteration.  lo, hi are in the solver's units, rounded inwards by the host (box_host.h).
// tall_tail_kernel's geometry: kTailElems coordinates per workgroup, kTailLanes lanes summing a coordinate's partials, no tile list, no
// LDS beyond the norm scratch.  The owner lane loads u_j, lo_j, hi_j beside the coordinate's other loads -- their addresses need
// nothing from the control block, so the launch is still one memory round trip.  The products of a discarded x-update are ignored
// exactly as tall_tail_kernel ignores them (mode 0 keeps the stored x; done returns), so the tiles' early exit stays on.
// Shared with the other tails as functions: tall_gather_ab, tall_soft, tall_extrapolate, tall_publish_norms.  The choice of
// (adj_z, adj_y, x) and the second half restate tall_update_elem and must be kept equal to it by hand (see the group tail); with
// u = 1 and infinite bounds every value here is tall_tail_kernel's, bit for bit.
struct BoxTailParams {
    const double* pf;                             // [p] penalty factors u_j
    const float* lo; const float* hi;             // [p] bounds in the solver's units (+-infinity: none)
};

template <int MODE>
__global__ void __launch_bounds__(kTailThreads)
tall_box_tail_kernel(TallParams q, int par, BoxTailParams bp) {
#pragma clang fp contract(off)
    static_assert(MODE == TAIL_GEMV || MODE == TAIL_SYMV || MODE == TAIL_SYMV1, "single device");
    __shared__ double scratch[6 * (kTailThreads / 64)];
    const TallCtl c = q.ctl[par ^ 1];
    const int sub = threadIdx.x & (kTailLanes - 1);
    const int i = blockIdx.x * kTailElems + threadIdx.x / kTailLanes;
    const bool valid = i < q.p;
    const bool owner = valid && sub == 0;
    TallElem e = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    double pf = 0.0;
    float lo = 0.f, hi = 0.f;
    if (owner) { e = tall_load_elem(q, par, i); pf = bp.pf[i]; lo = bp.lo[i]; hi = bp.hi[i]; }
    float a, b;
    tall_gather_ab<MODE>(q, i, sub, valid, a, b);
    if (c.done && c.fin_idx < 0) return;

    double acc[6] = {0, 0, 0, 0, 0, 0};
    if (owner) {
        float* zo_ = par ? q.z0 : q.z1; float* yo_ = par ? q.y0 : q.y1;
        const float zc = e.zc, yc = e.yc, zo = e.zo, yo = e.yo;
        if (c.fin_idx >= 0) q.beta[(size_t)c.fin_idx * q.p + i] = zc;     // get_z() snapshot (Lasso.cpp:108)
        if (!c.done) {
            float adjz, adjy, x;
            if (c.mode) {
                if (c.restart) { adjz = zo; adjy = yo; x = b; }
                else {
                    const float t = (float)c.tau, t1 = (float)(1.0 + c.tau);
                    adjz = tall_extrapolate(t1, t, zc, zo);
                    adjy = tall_extrapolate(t1, t, yc, yo);
                    x = a;
                }
            } else { adjz = e.adjz; adjy = e.adjy; x = e.x; }
            const float rho_f = (float)c.rho;
            const float vec = x + adjy / rho_f;
            const double pen = c.lam * pf / c.rho;
            float zn;
            if (!q.enet) zn = tall_soft(vec, pen);
            else {
                const float thresh = (float)(q.alpha * pen);
                const float denom = (float)(1.0 + pen * (1.0 - q.alpha));
                zn = vec > thresh ? (vec - thresh) / denom : (vec < -thresh ? (vec + thresh) / denom : 0.f);
            }
            zn = fminf(fmaxf(zn, lo), hi);
            const float r = x - zn;
            const float yn = adjy + rho_f * r;
            const float dz = zn - zc, daz = zn - adjz;
            acc[0] = (double)r * r; acc[1] = (double)dz * dz; acc[2] = (double)daz * daz;
            acc[3] = (double)x * x; acc[4] = (double)zn * zn; acc[5] = (double)yn * yn;
            q.x[i] = x; zo_[i] = zn; yo_[i] = yn; q.adj_z[i] = adjz; q.adj_y[i] = adjy;
            if (q.state != nullptr && c.total < q.state_cap) {
                float* s = q.state + (size_t)c.total * 5 * q.p;
                s[i] = x; s[q.p + i] = zn; s[2 * (size_t)q.p + i] = yn; s[3 * (size_t)q.p + i] = adjz; s[4 * (size_t)q.p + i] = adjy;
            }
            const float tn = (float)c.tau_next, tn1 = (float)(1.0 + c.tau_next);
            const float adjz_a = tall_extrapolate(tn1, tn, zn, zc), adjy_a = tall_extrapolate(tn1, tn, yn, yc);
            q.u[i] = (float)((double)(e.xy - adjy_a) + c.rho * (double)adjz_a);
            q.w[i] = (float)((double)(e.xy - yc) + c.rho * (double)zc);
        }
    }
    if (c.done) return;
    tall_publish_norms(q, par, acc, scratch);
}

// ---- multi-task lasso (admm_hip_mtlasso): m responses on ONE cached inverse, a row-wise block soft-threshold
//     Z_j. = V_j. max(0, 1 - pen_j / ||V_j.||_2),  V = X + adj_Y / rho,  pen_j = lambda w_j / rho
// The iterates are m planes (x, z, y, adj_z, adj_y: [m][ldv]; the right-hand sides u_k, w_k planes 2k, 2k + 1 of uw), the x-update is
// ceil(2m / NR) passes of symvn_lower_kernel (symv_kernels.h), each writing one plane of partials per right-hand side.  This tail has
// tall_tail_kernel<TAIL_SYMV>'s geometry -- 32 coordinates per workgroup, 8 lanes per coordinate summing partials -- and loops over the
// responses of its coordinate, kMtChunk at a time with the loads of a chunk issued together.  A row's m values belong to one owner lane:
// the row norm is the sum of (double) v_k^2 in the order k = 0 .. m - 1 in registers -- no LDS tiles, no tile list, no atomics.  The
// scalar threshold, the shrink factor and the norm sum are the other tails' functions (tall_soft, tall_block_shrink, tall_publish_norms);
// the choice of (adj_z, adj_y, x) and the second half restate tall_update_elem (see the group tail).  m = 1 takes tall_soft, and every
// sum is then tall_tail_kernel's: admm_hip_lasso bit for bit.
struct MtTailParams {
    int m;
    long long ldv, ldxy;                  // plane strides of the iterates and of X'Y
    float* uw;                            // [2m][ldv]
    const float* dot; const float* axp;   // partial planes [2m] of symvn_lower_kernel
    long long dot_stride, axp_stride;
    const double* row_w;                  // [p] row weights
};
constexpr int kMtMax = ADMM_HIP_MT_MAX;      // kMtChunk: symv_kernels.h
static_assert(kMtMax % kMtChunk == 0, "whole chunks");

__global__ void __launch_bounds__(kTailThreads)
tall_mt_tail_kernel(TallParams q, int par, MtTailParams mp) {
#pragma clang fp contract(off)
    __shared__ double scratch[6 * (kTailThreads / 64)];
    const TallCtl c = q.ctl[par ^ 1];
    const int sub = threadIdx.x & (kTailLanes - 1);
    const int i = blockIdx.x * kTailElems + threadIdx.x / kTailLanes;
    const bool valid = i < q.p;
    const bool owner = valid && sub == 0;
    const int m = mp.m;
    const float* zc_ = par ? q.z1 : q.z0; const float* yc_ = par ? q.y1 : q.y0;
    float* zo_ = par ? q.z0 : q.z1; float* yo_ = par ? q.y0 : q.y1;
    const double wj = owner ? mp.row_w[i] : 0.0;
    const float rho_f = (float)c.rho;
    // the row between the two halves of the update: x, adj_z, adj_y, v and what the second half still needs of the loads (registers: every index below is a constant once unrolled)
    float sx[kMtMax], sadjz[kMtMax], sadjy[kMtMax], sv[kMtMax], szc[kMtMax], syc[kMtMax], sxy[kMtMax];
    double nrm2 = 0.0;

    // ---- first half: x-update results, extrapolation, v = x + adj_y / rho, the row norm
#pragma unroll
    for (int ch = 0; ch < kMtMax / kMtChunk; ++ch) {
        const int k0 = ch * kMtChunk;
        if (k0 < m) {
            const int nk = min(kMtChunk, m - k0);
            TallElem e[kMtChunk];
#pragma unroll
            for (int kk = 0; kk < kMtChunk; ++kk) {
                const int kc = min(k0 + kk, m - 1);
                const size_t o = (size_t)kc * mp.ldv + i;
                e[kk] = TallElem{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                if (owner) {
                    e[kk].zc = zc_[o]; e[kk].yc = yc_[o]; e[kk].zo = zo_[o]; e[kk].yo = yo_[o];
                    e[kk].adjz = q.adj_z[o]; e[kk].adjy = q.adj_y[o]; e[kk].x = q.x[o]; e[kk].xy = q.XY[(size_t)kc * mp.ldxy + i];
                }
            }
            float a[kMtChunk], b[kMtChunk];
            symv_sum_partials_n<kTailLanes, kMtChunk>(mp.dot + (size_t)(2 * k0) * mp.dot_stride, mp.dot_stride, mp.axp + (size_t)(2 * k0) * mp.axp_stride, mp.axp_stride,
                                                      nk, q.ldo, q.nrb, q.sched, q.p32, i, sub, valid, a, b);
            if (c.done && c.fin_idx < 0) return;
#pragma unroll
            for (int kk = 0; kk < kMtChunk; ++kk) {
                const int k = k0 + kk;
                if (kk < nk && owner) {
                    const TallElem el = e[kk];
                    if (c.fin_idx >= 0) q.beta[((size_t)c.fin_idx * m + k) * q.p + i] = el.zc;     // snapshot beta[fin_idx][k][j]
                    if (!c.done) {
                        float adjz, adjy, x;
                        if (c.mode) {
                            if (c.restart) { adjz = el.zo; adjy = el.yo; x = b[kk]; }
                            else {
                                const float t = (float)c.tau, t1 = (float)(1.0 + c.tau);
                                adjz = tall_extrapolate(t1, t, el.zc, el.zo);
                                adjy = tall_extrapolate(t1, t, el.yc, el.yo);
                                x = a[kk];
                            }
                        } else { adjz = el.adjz; adjy = el.adjy; x = el.x; }
                        const float vec = x + adjy / rho_f;
                        sx[k] = x; sadjz[k] = adjz; sadjy[k] = adjy; sv[k] = vec; szc[k] = el.zc; syc[k] = el.yc; sxy[k] = el.xy;
                        const double v = (double)vec;
                        nrm2 += v * v;
                    }
                }
            }
        }
    }
    if (c.done) return;

    const double pen = c.lam * wj / c.rho;
    double shrink = 0.0;                                                // max(0, 1 - pen / ||v_j.||)
    if (m > 1) shrink = tall_block_shrink(nrm2, pen);

    // ---- second half: next_z, residual, dual update, norms, the right-hand sides of the next x-update (tall_update_elem's, restated)
    double acc[6] = {0, 0, 0, 0, 0, 0};
    const float tn = (float)c.tau_next, tn1 = (float)(1.0 + c.tau_next);
    const size_t pm = (size_t)q.p * m;
#pragma unroll
    for (int k = 0; k < kMtMax; ++k) {
        if (k < m && owner) {
            const float x = sx[k], adjz = sadjz[k], adjy = sadjy[k], vec = sv[k], zc = szc[k], yc = syc[k], xy = sxy[k];
            const double v = (double)vec;
            float zn;
            if (m == 1) zn = tall_soft(vec, pen);
            else zn = (float)(v * shrink);
            const float r = x - zn;
            const float yn = adjy + rho_f * r;
            const float dz = zn - zc, daz = zn - adjz;
            acc[0] += (double)r * r; acc[1] += (double)dz * dz; acc[2] += (double)daz * daz;
            acc[3] += (double)x * x; acc[4] += (double)zn * zn; acc[5] += (double)yn * yn;
            const size_t o = (size_t)k * mp.ldv + i;
            q.x[o] = x; zo_[o] = zn; yo_[o] = yn; q.adj_z[o] = adjz; q.adj_y[o] = adjy;
            if (q.state != nullptr && c.total < q.state_cap) {          // record [5][m][p]
                float* st = q.state + (size_t)c.total * 5 * pm + (size_t)k * q.p + i;
                st[0] = x; st[pm] = zn; st[2 * pm] = yn; st[3 * pm] = adjz; st[4 * pm] = adjy;
            }
            const float adjz_a = tall_extrapolate(tn1, tn, zn, zc), adjy_a = tall_extrapolate(tn1, tn, yn, yc);
            mp.uw[(size_t)(2 * k) * mp.ldv + i] = (float)((double)(xy - adjy_a) + c.rho * (double)adjz_a);
            mp.uw[(size_t)(2 * k + 1) * mp.ldv + i] = (float)((double)(xy - yc) + c.rho * (double)zc);
        }
    }
    tall_publish_norms(q, par, acc, scratch);
}

// Round 4 also built the whole path as ONE persistent launch with a third of the inverse's triangle resident in registers (two
// grid barriers per iteration, decision off the critical path; bit-identical): 66.7 us per iteration against 39.25 at C2 -- the
// barriers + an in-launch tail cost 16.6 us where the kernel boundaries cost 5.6, residency saves at most 10.8 us of the stream, and
// the stream itself falls to 2.5 TB/s with half the registers taken.  Measurements and the bound that rules out tuning it into a
// win: profiles/r04_tall_persist.md; the code: commit 6d31127.

// Row-sharded mode: this rank's share of the two products (the partial arrays of its tiles) summed into ab[2][ld], the
// vectors the ranks then all-reduce.  Same lane geometry and order as the single-GPU tail.
__global__ void __launch_bounds__(kTailThreads)
tall_shard_reduce_kernel(TallParams q, float* ab, long long ld, const int* skip) {
    if (*skip) return;
    const int sub = threadIdx.x & (kTailLanes - 1);
    const int i = blockIdx.x * kTailElems + threadIdx.x / kTailLanes;
    float a, b;
    symv_sum_partials<kTailLanes>(q.dot0, q.dot1, q.axp0, q.axp1, q.ldo, q.nrb, q.sched, q.p32, i, sub, i < q.p, a, b);
    if (i < q.p && sub == 0) { ab[i] = a; ab[ld + i] = b; }
}

// Refined x-update, residual step: r = rhs - M x1 for both candidates, M x1 from the double partial arrays of
// symv2_lower_f64acc_kernel, the subtraction in double, the result rounded to float once.
__global__ void __launch_bounds__(kTailThreads)
tall_refine_resid_kernel(TallParams q, const double* d0, const double* d1, const double* x0, const double* x1, float* ru, float* rw, const int* skip) {
    if (*skip) return;
    const int sub = threadIdx.x & (kTailLanes - 1);
    const int i = blockIdx.x * kTailElems + threadIdx.x / kTailLanes;
    double ma, mb;
    symv_sum_partials<kTailLanes, double>(d0, d1, x0, x1, q.ldo, q.nrb, q.sched, q.p32, i, sub, i < q.p, ma, mb);
    if (i < q.p && sub == 0) { ru[i] = (float)((double)q.u[i] - ma); rw[i] = (float)((double)q.w[i] - mb); }
}

// The same over the PEER exchange, without launches of the exchange layer: every workgroup writes its elements of
// (a, b) straight into this rank's slot of EVERY rank's buffer (lane `sub` of an element's group serves rank sub,
// sub + 8, ...), and the last workgroup to finish raises the flags (peer_device.h).
__global__ void __launch_bounds__(kTailThreads)
tall_shard_push_kernel(TallParams q, PeerExchange ex, long long ld, const int* skip) {
    if (*skip) return;
    const int sub = threadIdx.x & (kTailLanes - 1);
    const int i = blockIdx.x * kTailElems + threadIdx.x / kTailLanes;
    float a, b;
    symv_sum_partials<kTailLanes>(q.dot0, q.dot1, q.axp0, q.axp1, q.ldo, q.nrb, q.sched, q.p32, i, sub, i < q.p, a, b);
    if (i < q.p) {
        for (int dst = sub; dst < ex.nranks; dst += kTailLanes)
            peer_store_f32x2(reinterpret_cast<float*>(peer_dst_slot(ex, dst)) + 2 * (size_t)i, a, b);       // (a_i, b_i) interleaved: one 8-byte store
    }
    peer_publish(ex, gridDim.x);
}

__global__ void tall_init_kernel(TallParams q, double rho, double lam0) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < q.p) {
        q.x[i] = 0.f; q.z0[i] = 0.f; q.z1[i] = 0.f; q.y0[i] = 0.f; q.y1[i] = 0.f;
        q.adj_z[i] = 0.f; q.adj_y[i] = 0.f; q.u[i] = q.XY[i]; q.w[i] = 0.f;
    }
    if (i < 2 * q.nwg * (8 + kGateCols)) q.P[i] = 0.0;
    if (i == 0) {
        TallCtl c;
        c.rho = rho; c.lam = lam0; c.eps_primal = 0.0; c.eps_dual = 0.0;
        c.adj_a = 1.0; c.adj_c = 9999.0; c.tau = 0.0;
        c.a_next = 0.5 + 0.5 * sqrt(5.0); c.tau_next = 0.0;
        c.mode = 1; c.restart = 0; c.iter = 0; c.lam_idx = 0; c.done = 0; c.first = 1; c.total = 0; c.fin_idx = -1; c.fin_niter = 0; c.pad = 0;
        q.ctl[0] = c; q.ctl[1] = c;
        if (q.early != nullptr)                    // tiles that left early in this run (the verdict words themselves carry the run number)
            for (int k = 0; k < kSyEarlySlots; ++k) q.early[(size_t)k * kSyVerdictStride] = 0;
    }
}

// Tiles of the x-update that left early in the calling thread's most recent tall path (test hook admm_hip_test_tall_early_exits).
static thread_local long long t_early_exits = 0;
long long tall_last_early_exits() { return t_early_exits; }
// The calling thread's most recent tall plan: 1 if its x-update streams the 29-bit copy, escapes met while packing, tiles whose escape list
// overflowed, bytes of the copy (all 0 where no copy was attempted).
static thread_local long long t_pack_info[4] = {0, 0, 0, 0};
void tall_last_pack_info(long long* out) { for (int k = 0; k < 4; ++k) out[k] = t_pack_info[k]; }

// Test hooks admm_hip_test_tall_gate / admm_hip_test_tall_norms: the decision as ONE tile takes it (TallGate's request, sums and decide on
// the compact copy of the norm partials) and the six sums as block 0 forms them from the rows of P, each by one workgroup of the kernels'
// size on caller-supplied inputs.  The two must agree to the bit in the first three sums: a tile that decided otherwise than block 0
// would multiply the wrong vector.
__global__ void __launch_bounds__(kSyThreads) tall_gate_hook_kernel(TallGate gate, double* sums_out, int* answer_out) {
    __shared__ double lds[kSyGateScratch];
    const TallGate::Req r = gate.request();
    double acc[kGateCols];
    gate.sums(r, lds, acc);
    const int g = gate.decide(r, lds);
    if (threadIdx.x == 0) {
        for (int k = 0; k < kGateCols; ++k) sums_out[k] = acc[k];
        *answer_out = g;
    }
}
__global__ void __launch_bounds__(kTailThreads) tall_norms_hook_kernel(const double* rows, int nwg, double* sums_out) {
    __shared__ double lds[6 * (kTailThreads / 64)];
    double acc[6];
    tall_norms_sum<6, false>(tall_norms_request<6, false>(rows, nwg, 8, 1), rows, nwg, 8, 1, acc, lds);
    if (threadIdx.x == 0) { for (int k = 0; k < 6; ++k) sums_out[k] = acc[k]; }
}
void test_tall_gate(const double* ctl_d, const int* ctl_i, const double* compact, int nwg, int maxit, int nlam, double* sums_out, int* answer_out) {
    Stream st;
    TallCtl c;
    c.rho = ctl_d[0]; c.lam = ctl_d[1]; c.eps_primal = ctl_d[2]; c.eps_dual = ctl_d[3]; c.adj_a = ctl_d[4]; c.adj_c = ctl_d[5]; c.tau = ctl_d[6];
    c.a_next = ctl_d[7]; c.tau_next = ctl_d[8];
    c.mode = ctl_i[0]; c.restart = ctl_i[1]; c.iter = ctl_i[2]; c.lam_idx = ctl_i[3]; c.done = ctl_i[4]; c.first = ctl_i[5]; c.total = ctl_i[6];
    c.fin_idx = ctl_i[7]; c.fin_niter = ctl_i[8]; c.pad = 0;
    DevBuf<TallCtl> dc(1);
    DevBuf<double> dP((size_t)kGateCols * nwg), ds(kGateCols);
    DevBuf<int> da(1);
    ADMM_HIP_CHECK(hipMemcpyAsync(dc.get(), &c, sizeof(TallCtl), hipMemcpyHostToDevice, st.s));
    ADMM_HIP_CHECK(hipMemcpyAsync(dP.get(), compact, (size_t)kGateCols * nwg * sizeof(double), hipMemcpyHostToDevice, st.s));
    ADMM_HIP_CHECK(hipStreamSynchronize(st.s));       // (c is on this frame)
    const TallGate gate = {dc.get(), dP.get(), nwg, maxit, nlam};
    hipLaunchKernelGGL(tall_gate_hook_kernel, dim3(1), dim3(kSyThreads), 0, st.s, gate, ds.get(), da.get());
    ADMM_HIP_CHECK(hipGetLastError());
    read_back(sums_out, ds.get(), kGateCols * sizeof(double), st.s);
    read_back(answer_out, da.get(), sizeof(int), st.s);
}
void test_tall_norms(const double* rows, int nwg, double* sums_out) {
    Stream st;
    DevBuf<double> dP((size_t)8 * nwg), ds(6);
    ADMM_HIP_CHECK(hipMemcpyAsync(dP.get(), rows, (size_t)8 * nwg * sizeof(double), hipMemcpyHostToDevice, st.s));
    hipLaunchKernelGGL(tall_norms_hook_kernel, dim3(1), dim3(kTailThreads), 0, st.s, dP.get(), nwg, ds.get());
    ADMM_HIP_CHECK(hipGetLastError());
    read_back(sums_out, ds.get(), 6 * sizeof(double), st.s);
}

// ----------------------------------------------------------------------------------------------
struct TallPlan final : LassoPlan {
    DeviceData<float> d;
    LassoProblem pb;
    hipStream_t st;
    admm_stats setup_stats{};
    int p = 0, nlam = 0, nwg = 0;
    long long ldp = 0;
    double rho = 0;
    std::vector<double> lam_user, lam_int;
    GemvTPlan pl;
    SymvPlan sy;
    bool use_sym = false;
    bool shard = false;                                 // x-update spread over the ranks of the attached communicator
    bool peer_fused = false;                            // ... with the exchange done by the solver's own kernels (PEER backend)
    bool peer_one = false;                              // ... producer and consumer in one launch (tall_tail_kernel<TAIL_PEER1>)
    int exchange_code = 0;                              // ... as admm_stats.exchange_variant reports it
    CommInfo ci;
    DevBuf<float> ab;                                   // [2][ldp] this rank's share of (a, b), all-reduced in place
    double dist_flops = 0;                              // distributed factorisation: flops this rank performed (0: replicated)
    long long ldv = 0;
    DevBuf<float> XY, M, a_part, b_part, x, z0, z1, y0, y1, adj_z, adj_y, u, w, beta;
    DevBuf<int> niter;
    DevBuf<double> P, dlam;
    DevBuf<TallCtl> ctl;
    DevBuf<unsigned long long> verdict;                 // early exit of discarded x-update launches (symv_kernels.h: SymvVerdict): the words + the counter
    bool verdict_on = false, verdict_mid = false;
    bool decide_first = false;                          // SYMV_VERDICT=3 (default): every tile takes the decision itself and multiplies one vector (symv1_lower_kernel, TAIL_SYMV1)
    SymvPacked pk;                                      // SYMV_PACK=1 (default): the exact 29-bit copy of the tiles the decide-first x-update streams (symv_pack.h)
    bool packed = false;                                // ... is in use (false: the fp32 stream -- option off, no memory for the copy, or a tile's escape list overflowed)
    unsigned long long run_no = 0;                      // run() calls of this plan: part of the verdict word
    TallParams q{};
    // mixed-precision refinement of the x-update (ADMM_HIP_REFINE=1)
    bool refine = false;
    DevBuf<float> Mg, rab, ruw;                          // the float system X'X + rho I; first solve a | b; residuals r_u | r_w
    DevBuf<double> dD0, dD1, xD0, xD1;                   // double partial arrays of M x1
    // group and sparse-group lasso (Penalty::GROUP, SGL): the tail is tall_group_tail_kernel over tiles of whole groups, nwg = their number
    bool grouped = false, sgl = false;
    DevBuf<int2> gtiles;
    DevBuf<GroupCoord> gcoord;
    DevBuf<double> gl1;                                 // sparse-group lasso: the l1 weight of every column
    GroupTailParams gq{};
    // multi-task lasso (Penalty::MULTITASK): every vector is nresp planes, the x-update passes of symvn_lower_kernel, the tail tall_mt_tail_kernel
    int mt = 0;                                         // responses (0: not a multi-task problem)
    int mt_rhs = 2;                                     // right-hand sides per pass (MT_RHS)
    DevBuf<float> uw, mdot, maxp;                       // [2 mt][ldv] right-hand sides; [2 mt] planes of partials
    DevBuf<double> roww;
    MtTailParams mq{};
    // box-constrained, weighted elastic net (Penalty::BOX): factors and bounds of every column, the tail tall_box_tail_kernel
    bool box = false;
    DevBuf<double> bpf;
    DevBuf<float> blo, bhi;                             // the bounds in the solver's units, rounded inwards (box_host.h)
    BoxTailParams bq{};
    BoxClamp clamp;                                     // the caller's bounds for the recovered coefficients
    PinnedFlag hflag;
#ifdef ADMM_HIP_PROBE
    DevBuf<long long> probe;
#endif
    float* hbeta = nullptr;                             // pinned landing buffer of the beta snapshots (nlam x p)

    std::vector<hipEvent_t> ev_pool;                    // start/stop events of sampled x-update launches, reused by every run()

    ~TallPlan() override {
        if (hbeta) (void)hipHostFree(hbeta);
        for (auto e : ev_pool) (void)hipEventDestroy(e);
    }

    TallPlan(DeviceData<float>&& data, const LassoProblem& prob, hipStream_t stream) : d(std::move(data)), pb(prob), st(stream) {
        const int n = d.n;
        p = d.p;
        admm_stats& S = setup_stats;
        S.branch = 0;
        S.t_h2d = d.t_h2d; S.t_standardize = d.t_std;
        ldp = round_up(p, 128);                         // whole 128-row blocks for the matrix-core setup kernels

        // X'y and lambda_0 (ADMMLassoTall.h:172-173; ADMMEnet.h:56 divides by alpha + 1e-4)
        // Row-sharded mode (not in the reference): d holds this rank's ROWS of the globally standardised
        // data.  X'y and X'X are sums over the row blocks (split-K over the ranks + one all-reduce each); the Lanczos call
        // and the factorisation are replicated (identical inputs -> identical rho and inverse on every rank); each rank
        // then streams 1/nranks of the inverse's lower-triangle tiles per iteration.
        shard = pb.dist;
        ci = shard ? comm_info() : CommInfo();
        const long long nt = d.n_total > 0 ? d.n_total : n;
        if (d.xy.get()) {                                  // Gram-form data (a cross-validation fold formed as a down-date, cv.hip)
            ADMM_REQUIRE(!shard && d.gram.get() && d.ldgram == ldp, "Gram-form data needs X'X next to X'y");
            XY = std::move(d.xy);
        } else if (pb.penalty == Penalty::MULTITASK) {     // X'Y, one plane per response
            mt = pb.nresp;
            ADMM_REQUIRE(mt >= 1 && mt <= kMtMax && d.nresp == mt && d.Ymt.get() && (int)pb.row_weight.size() == p, "internal: multi-task sizes");
            XY.alloc((size_t)mt * ldp); XY.zero(st);
            for (int k = 0; k < mt; ++k) gemv_t_simple<float>(d.X.get(), d.ldx, n, p, d.Ymt.get() + (size_t)k * d.ldx, XY.get() + (size_t)k * ldp, st);
        } else {
            XY.alloc(ldp); XY.zero(st);
            gemv_t_simple<float>(d.X.get(), d.ldx, n, p, d.Y.get(), XY.get(), st);
            if (shard) allreduce_sum_f32(XY.get(), (size_t)p, st);
        }
        sgl = pb.penalty == Penalty::SGL; grouped = sgl || pb.penalty == Penalty::GROUP; box = pb.penalty == Penalty::BOX;
        ADMM_REQUIRE(pb.penalty == Penalty::PLAIN || (!shard && !opt_on(Opt::REFINE) && (box || !pb.enet) && (mt > 0) == (pb.penalty == Penalty::MULTITASK)),
                     "internal: a penalty other than the Lasso's is the plain single-device tall solver on column data");
        ADMM_REQUIRE(!grouped || ((int)pb.group_start.size() == (int)pb.group_weight.size() + 1 && pb.group_start.back() == p), "internal: group sizes");
        ADMM_REQUIRE((int)pb.l1_weight.size() == (sgl ? p : 0), "internal: l1 weights belong to the sparse-group lasso");
        ADMM_REQUIRE(!box || ((int)pb.box_lower.size() == p && (int)pb.box_upper.size() == p && (int)pb.penalty_factor.size() == p), "internal: box sizes");
        float lambda0 = 0.f;
        switch (pb.penalty) {
        case Penalty::PLAIN: lambda0 = device_absmax<float>(XY.get(), p, st); break;
        case Penalty::GROUP: lambda0 = group_lambda0(); break;
        case Penalty::SGL: lambda0 = sgl_plan_lambda0(); break;
        case Penalty::MULTITASK: lambda0 = mt_lambda0(); break;
        case Penalty::BOX: lambda0 = box_plan_lambda0(); break;
        }
        if (pb.enet) lambda0 = (float)(lambda0 / ((double)(float)pb.alpha + 0.0001));

        // lambda grid (Lasso.cpp:78-89) and internal lambdas (Lasso.cpp:99), stored as float like `Scalar lambda`
        nlam = make_path_grid<float>(pb, lambda0, nt, (double)d.scaleY, lam_user, lam_int);

        // Memory wall: this solver keeps (X'X + rho I)^-1, ldp^2 floats, next to X (until the loop starts), the Gram and -- below
        // p = 4096 or with ADMM_HIP_INVERSE=f64 -- a double copy during the factorisation.  Refuse clearly instead of failing
        // inside some allocation (ADMM_HIP_TEST_FREE_BYTES: test hook that pretends the device has that much memory left).
        {
            size_t free_b = 0, total_b = 0;
            ADMM_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
            free_b += pool_cached_bytes();                        // blocks this library holds for re-use are free for it
            if (opt_set(Opt::TEST_FREE_BYTES)) free_b = (size_t)opt_int(Opt::TEST_FREE_BYTES, 0);
            const bool have_gram = d.gram.get() && d.ldgram == ldp;
            const bool inv64_wanted = p < 4096 || opt_is(Opt::INVERSE, "f64");
            const double mat = (double)ldp * (double)ldp * 4.0;
            const double need = (have_gram ? 0.0 : mat) + (inv64_wanted ? 2.0 * mat : 0.5 * mat) + (opt_on(Opt::REFINE) ? mat : 0.0) +
                                (shard && ci.nranks > 1 ? mat + mat / ci.nranks : 0.0) +     // packed send / receive buffers of the Gram's reduce-scatter
                                (mt ? mt_partial_floats() * 4.0 : 0.0);                      // multi-task: a plane of partials per right-hand side
            if (need > 0.97 * (double)free_b) {
                char msg[320];
                std::snprintf(msg, sizeof msg, "tall solver: the cached %d x %d inverse and its workspace need %.1f GB, the device has %.1f GB free; "
                              "use $parallel() (row blocks, admm_hip_parlasso) or fewer columns", p, p, need / 1e9, (double)free_b / 1e9);
                throw Error(ADMM_ERR_MEMORY, msg);
            }
        }
        // Gram (cross_prod_lower, ADMMLassoTall.h:191-192) -- both triangles
        double t0 = now_s();
        const bool gram_given = d.gram.get() && d.ldgram == ldp;
        if (gram_given) {                                 // computed under the host-to-device transfer (upload_standardize_gram_f32)
            M = std::move(d.gram);
            S.t_gram = d.t_gram_tail;
        } else {
            M.alloc((size_t)ldp * ldp); M.zero(st);
            gram_full<float>(d.X.get(), d.ldx, n, p, true, M.get(), ldp, st);      // sharded: this rank's term of the split-K sum (reduced below)
            comm_stream_sync(st);
            S.t_gram = now_s() - t0;
        }
        // Row-sharded solver: decided here because it chooses how the split-K Gram is reduced (below)
        bool inv64 = p < 4096;
        if (opt_set(Opt::INVERSE)) inv64 = opt_is(Opt::INVERSE, "f64");
        bool dist_factor = shard && ci.nranks > 1 && !inv64 && (p + 127) / 128 >= 2 * ci.nranks && p >= 256;
        if (opt_off(Opt::DIST_FACTOR)) dist_factor = false;

        // rho (ADMMLassoTall.h:194-202)
        rho = pb.opts.rho;
        t0 = now_s();
        if (rho <= 0) {
            SymMatVec<float> op(M.get(), ldp, p, st);
            int nmatop = 0;
            // Row-sharded: M still holds this rank's term X_r'X_r of the Gram, and the product is (sum_r X_r'X_r) v = sum_r (X_r'X_r v):
            // the local product, then ONE all-reduce of p floats per Lanczos step (3-5 steps) -- so the whole matrix never has to exist
            // on any rank (round 3 all-reduced the p x p Gram first).  Identical sums in identical order on every rank: identical rho.
            DevBuf<float> wsum;
            if (shard && ci.nranks > 1) wsum.alloc(ldp);
            const float ev = lanczos_largest_f32([&](const float* v, float* w_) {
                op(v, w_);
                if (shard && ci.nranks > 1) {
                    ADMM_HIP_CHECK(hipMemcpyAsync(wsum.get(), w_, (size_t)p * sizeof(float), hipMemcpyHostToDevice, st));
                    allreduce_sum_f32(wsum.get(), (size_t)p, st);
                    ADMM_HIP_CHECK(hipMemcpyAsync(w_, wsum.get(), (size_t)p * sizeof(float), hipMemcpyDeviceToHost, st));
                    comm_stream_sync(st);
                    comm_check();
                }
            }, p, &nmatop);
            S.eig_est = ev;
            rho = std::pow((double)ev, 1.0 / 3) * std::pow(lam_int[0], 2.0 / 3);
        }
        S.rho = rho;
        S.t_eigs = now_s() - t0;

        // Row-sharded: the split-K sum of the Gram over the ranks.  With the distributed factorisation a rank
        // only ever reads the block columns it owns (k mod N == rank: chol_inverse.h), so the sum is a REDUCE-SCATTER: the block columns
        // are packed owner by owner (a block column is 128 x ldp contiguous floats), every rank receives the sum of its own -- 1 / N of the
        // matrix -- and unpacks it in place; the other block columns of M are dead from here on (the panels arrive by broadcast).
        // Replicated factorisation (ADMM_HIP_DIST_FACTOR=0, double-built inverses, few blocks): the all-reduce of round 3.
        if (shard && ci.nranks > 1 && !gram_given) {            // (a Gram that arrived with the data is a single-process set-up: never sharded)
            const double tr0 = now_s();
            if (dist_factor) {
                const int nb128 = (p + 127) / 128, N = ci.nranks;
                const int nown = (nb128 + N - 1) / N;                           // slots per rank (the last ones of some ranks stay zero)
                const size_t blk = (size_t)128 * ldp, cnt = (size_t)nown * blk;
                DevBuf<float> send((size_t)N * cnt), recv(cnt);
                send.zero(st);
                for (int k = 0; k < nb128; ++k) {
                    const size_t cols = (size_t)std::min(128, (int)ldp - k * 128);
                    ADMM_HIP_CHECK(hipMemcpyAsync(send.get() + ((size_t)(k % N) * nown + k / N) * blk, M.get() + (size_t)k * blk, cols * ldp * sizeof(float),
                                                  hipMemcpyDeviceToDevice, st));
                }
                reduce_scatter_sum_f32(send.get(), recv.get(), cnt, st);
                for (int k = ci.rank; k < nb128; k += N) {
                    const size_t cols = (size_t)std::min(128, (int)ldp - k * 128);
                    ADMM_HIP_CHECK(hipMemcpyAsync(M.get() + (size_t)k * blk, recv.get() + (size_t)(k / N) * blk, cols * ldp * sizeof(float), hipMemcpyDeviceToDevice, st));
                }
            } else {
                allreduce_sum_f32(M.get(), (size_t)ldp * ldp, st);
            }
            comm_stream_sync(st);
            comm_check();
            S.t_gram += now_s() - tr0;
        }

        // (X'X + rho I)^-1, cached for the whole path (rho never changes: ADMMLassoTall.h:97)
        // ADMM_HIP_INVERSE=f32: factorise and invert in float (the reference's LLT is a float factorisation, XX.diagonal() += rho in float).
        // ADMM_HIP_INVERSE=f64: the same float Gram factorised and inverted in double, rounded to float once -- each entry
        // of the cached inverse then carries half an ulp instead of cond * ulp (useful when n ~ p); it costs 150 ms more at
        // p = 10^4 and does not change how often the stopping rule flips against a float Cholesky solve (measured with
        // tests/tools/flip_floor.py: 45 vs 44 of 185 lambdas, the reference's own solve against the exact one: 39).
        // ADMM_HIP_REFINE=1 (opt-in): every x-update is refined once, x = x1 + Minv (rhs - M x1) with the residual in double
        // from the float system M = X'X + rho I (the reference's: XX.diagonal() += rho in float, ADMMLassoTall.h:204) -- the
        // x-update's error against the exact solve of that system drops from cond(M) ulps to about one ulp, i.e. onto what
        // oracle/variants.py calls the `exact` variant, at three passes over the triangle per iteration instead of one.
        refine = opt_on(Opt::REFINE) && !shard;
        if (refine) {
            Mg.alloc((size_t)ldp * ldp);
            ADMM_HIP_CHECK(hipMemcpyAsync(Mg.get(), M.get(), (size_t)ldp * ldp * sizeof(float), hipMemcpyDeviceToDevice, st));
            add_diag<float>(Mg.get(), ldp, p, (float)rho, st);
        }
        t0 = now_s();
        // Policy: double below p = 4096 (a few ms there, and the float inverse is 30-100x less accurate: 1-3e-6 against
        // 3e-8 of the largest entry at cond ~ 30, tests/test_gpu_kernels.py), float above.
        // Row-sharded solver: the factorisation's block columns dealt out to the ranks, and of the inverse
        // only the tiles this rank's share of the x-update reads -- 1 / N of the 2 p^3 / 3 + p^3 / 3 flops per rank, bit-identical to the
        // replicated factorisation (chol_inverse.h).  ADMM_HIP_DIST_FACTOR=0: every rank factorises the whole matrix (round 3).
        if (inv64) {
            spd_inverse_f32_via_f64(M.get(), ldp, p, (double)(float)rho, st);
        } else if (dist_factor) {
            add_diag<float>(M.get(), ldp, p, (float)rho, st);
            sy.init(p, st, ci.rank, ci.nranks);               // (the tile list of this rank's share; initialised again below, identically)
            std::vector<int> need;
            {
                const int nb128 = (p + 127) / 128;
                std::vector<char> mark((size_t)nb128 * nb128, 0);
                for (const int4& t : sy.htiles)
                    for (int bi = 2 * t.x; bi <= 2 * t.x + 1 && bi < nb128; ++bi)
                        for (int bj = t.y / 128; bj <= (t.y + t.z - 1) / 128 && bj < nb128; ++bj)
                            if (bj <= bi && !mark[(size_t)bi * nb128 + bj]) { mark[(size_t)bi * nb128 + bj] = 1; need.push_back(bi << 16 | bj); }
            }
            double fl = 0;
            spd_inverse_mfma_f32_dist(M.get(), ldp, p, need, &fl, st);
            dist_flops = fl;
        } else {
            add_diag<float>(M.get(), ldp, p, (float)rho, st);
            spd_inverse_f32(M.get(), ldp, p, st);
        }
        comm_stream_sync(st);
        S.t_factor = now_s() - t0;
        // X itself is no longer needed by the loop (only X'y and Minv are): release 4np bytes.
        d.X.release();

        // ---- loop state
        // x-update variant: lower-triangle symmetric mat-vec (2p^2 bytes) for large p, full-matrix
        // gemv_t (4p^2 bytes, fewer and larger workgroups) for small p.  ADMM_HIP_XUPDATE=sym|gemv|full overrides.
        use_sym = p >= 2048;
        if (opt_set(Opt::XUPDATE)) use_sym = opt_is(Opt::XUPDATE, "sym");
        if (refine) use_sym = true;                      // the refinement is built on the symmetric kernel's partial layout
        if (shard) use_sym = true;                       // the sharded x-update is the tile list of the symmetric kernel dealt out to the ranks
        if (mt) use_sym = true;                          // the multi-vector kernel is the symmetric one at every p: there is no gemv form
        pl = plan_gemv_t<float>(p, p, 2, 4);
        nwg = (p + kTailElems - 1) / kTailElems;
        if (grouped) nwg = pack_group_tiles();
        ldv = round_up(p, 256);                         // symv reads the right-hand vectors in 256-row blocks
        if (use_sym) sy.init(p, st, shard ? ci.rank : 0, shard ? ci.nranks : 1);
        if (refine) {
            rab.alloc((size_t)2 * ldv); rab.zero(st);
            ruw.alloc((size_t)2 * ldv); ruw.zero(st);
            dD0.alloc((size_t)sy.nrb * sy.ldo); dD1.alloc((size_t)sy.nrb * sy.ldo);
            xD0.alloc((size_t)sy.nax_rows * sy.ldo); xD1.alloc((size_t)sy.nax_rows * sy.ldo);
            dD0.zero(st); dD1.zero(st); xD0.zero(st); xD1.zero(st);
        }
        if (shard) { ab.alloc((size_t)2 * ldp); ab.zero(st); }
        else if (!use_sym) { a_part.alloc((size_t)pl.nseg * ldp); b_part.alloc((size_t)pl.nseg * ldp); a_part.zero(st); b_part.zero(st); }
        const ExchangeForm xf = peer_exchange_form(shard, ci, reinterpret_cast<const void*>(tall_tail_kernel<TAIL_PEER1>), kTailThreads, nwg);
        peer_fused = xf.fused; peer_one = xf.one; exchange_code = xf.variant;
        // (A single-launch iteration -- tail, decision and tiles in one launch -- and a hipGraph replay of the batch were built, measured
        // bit-identical and SLOWER on C2 in rounds 4 / 5 (44.5 and 46.9 us per iteration against 42.1 / 46.6): removed in round 6,
        // profiles/HISTORY.md.)
        const size_t npl = (size_t)std::max(mt, 1);     // planes per vector
        x.alloc(npl * ldv); z0.alloc(npl * ldv); z1.alloc(npl * ldv); y0.alloc(npl * ldv); y1.alloc(npl * ldv);
        adj_z.alloc(npl * ldv); adj_y.alloc(npl * ldv); u.alloc(ldv); w.alloc(ldv);
        beta.alloc((size_t)nlam * p * npl); niter.alloc(nlam);
        P.alloc((size_t)2 * nwg * (8 + kGateCols)); dlam.alloc(nlam); ctl.alloc(2);
        u.zero(st); w.zero(st);
        ADMM_HIP_CHECK(hipMemcpyAsync(dlam.get(), lam_int.data(), nlam * sizeof(double), hipMemcpyHostToDevice, st));

        q.p = p; q.nwg = nwg; q.nseg = pl.nseg; q.maxit = pb.opts.maxit; q.nlam = nlam; q.enet = pb.enet ? 1 : 0;
        q.part_stride = ldp;
        q.eps_abs = pb.opts.eps_abs; q.eps_rel = pb.opts.eps_rel; q.alpha = (double)(float)pb.alpha; q.sqrt_p = std::sqrt((double)p * (double)npl);
        q.lambdas = dlam.get(); q.XY = XY.get(); q.a_part = a_part.get(); q.b_part = b_part.get();
        if (shard) { q.a_part = ab.get(); q.b_part = ab.get() + ldp; q.nseg = 1; }      // the tail reads the all-reduced pair (generic exchange)
        q.dot0 = sy.dot0.get(); q.dot1 = sy.dot1.get(); q.axp0 = sy.axp0.get(); q.axp1 = sy.axp1.get();
        q.ldo = sy.ldo; q.nrb = sy.nrb; q.p32 = sy.p32; q.sched = sy.sched;
        q.refine_ab = refine ? rab.get() : nullptr; q.refine_ld = ldv;
        q.x = x.get(); q.z0 = z0.get(); q.z1 = z1.get(); q.y0 = y0.get(); q.y1 = y1.get();
        q.adj_z = adj_z.get(); q.adj_y = adj_y.get(); q.u = u.get(); q.w = w.get();
        q.ctl = ctl.get(); q.P = P.get(); q.beta = beta.get(); q.niter = niter.get();
        q.done_host = hflag.p;
        // Tiles leave early only where the tail provably ignores the products of a discarded launch: the single-device, unrefined
        // two-launch forms (tall_tail_kernel<TAIL_SYMV>, tall_group_tail_kernel<TAIL_SYMV>, tall_box_tail_kernel<TAIL_SYMV>).  Sharded, refined and multi-task x-updates
        // have consumers of their own between the stream and the tail.  ADMM_HIP_SYMV_VERDICT=3 (default): the tiles take the decision themselves before they
        // stream, and stream one vector (symv1_lower_kernel); 2 / 1: two vectors, and the tiles look for the verdict word block 0 publishes, between the
        // chunks of their column loop as well / in their prologue only; 0: two vectors, no tile ever leaves (A/B, tests).
        const int level = (int)opt_int(Opt::SYMV_VERDICT, 3);
        verdict_on = use_sym && !shard && !refine && !mt && level != 0;
        decide_first = verdict_on && level == 3;
        verdict_mid = level == 2;
        if (verdict_on) {
            verdict.alloc(kVerdictWords + kSyEarlySlots * kSyVerdictStride); verdict.zero(st);
            q.verdict = decide_first ? nullptr : verdict.get();      // decide-first: nobody reads a word, block 0 publishes none
            q.early = verdict.get() + kVerdictWords;
        }
        // The decide-first x-update streams an exact 29-bit copy of the inverse's tiles (symv1_packed_kernel: 29/32 of the bytes, the same 32 bits
        // after the decode, so nothing downstream changes).  Packed once here: the inverse and the tile list are fixed for the life of the
        // plan.  The fp32 stream stays when the option is off, the copy does not fit the device, or a tile has more entries outside its
        // exponent window than its list holds.
        packed = false;
        t_pack_info[0] = t_pack_info[1] = t_pack_info[2] = t_pack_info[3] = 0;
        if (decide_first && opt_int(Opt::SYMV_PACK, 1) != 0) {
            size_t free_b = 0, total_b = 0;
            ADMM_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
            free_b += pool_cached_bytes();
            if (opt_set(Opt::TEST_FREE_BYTES)) free_b = (size_t)opt_int(Opt::TEST_FREE_BYTES, 0);
            if ((double)SymvPacked::bytes_for(sy) <= 0.97 * (double)free_b) {
                packed = pk.build(sy, M.get(), ldp, st, (int)opt_int(Opt::SYMV_PACK_ESC, kSpEscCap));
                t_pack_info[1] = (long long)pk.escapes; t_pack_info[2] = (long long)pk.overflowed; t_pack_info[3] = (long long)pk.bytes();
                if (!packed) pk.release();
            }
            t_pack_info[0] = packed ? 1 : 0;
        }
#ifdef ADMM_HIP_PROBE
        probe.alloc((size_t)4096 * 4 * 8); probe.zero(st);
        q.probe = probe.get();
        sy.probe = probe.get();
#endif

        if (mt) {
            // right-hand sides per pass: MT_RHS, or the automatic value = the fastest measured at p = 10^4 for that m, every m from 1 to
            // 16 measured (scripts/bench_mtlasso.py, profiles/mtlasso_rhs.md).  A pass costs the same full or partly filled: about 31 us
            // for 2 or 4 vectors (the stream is the bound), 58 - 60 for 8 and 83 - 87 for 12 (the FMAs are), so the winner is the NR whose
            // ceil(2m / NR) passes waste the fewest slots -- no monotone rule in m.
            static const int kAutoRhs[kMtMax] = {2, 4, 8, 8, 12, 12, 8, 8, 4, 4, 12, 12, 4, 4, 8, 8};
            mt_rhs = kAutoRhs[mt - 1];
            if (const OptValue* v = opt(Opt::MT_RHS)) { if (v->i > 0) mt_rhs = kSyNR[v->i - 1]; }
            uw.alloc((size_t)2 * mt * ldv); uw.zero(st);
            const size_t ds = (size_t)sy.nrb * sy.ldo, as = (size_t)sy.nax_rows * sy.ldo;
            mdot.alloc((size_t)2 * mt * ds); maxp.alloc((size_t)2 * mt * as);
            mdot.zero(st); maxp.zero(st);
            x.zero(st); z0.zero(st); z1.zero(st); y0.zero(st); y1.zero(st); adj_z.zero(st); adj_y.zero(st);      // (the padding of the planes)
            roww.alloc(p);
            ADMM_HIP_CHECK(hipMemcpyAsync(roww.get(), pb.row_weight.data(), (size_t)p * sizeof(double), hipMemcpyHostToDevice, st));
            mq.m = mt; mq.ldv = ldv; mq.ldxy = ldp; mq.uw = uw.get();
            mq.dot = mdot.get(); mq.axp = maxp.get(); mq.dot_stride = (long long)ds; mq.axp_stride = (long long)as;
            mq.row_w = roww.get();
        }
        ADMM_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&hbeta), (size_t)nlam * p * npl * sizeof(float), hipHostMallocDefault));
        comm_stream_sync(st);
    }

    // The box-constrained elastic net's set-up: the caller's bounds into the solver's units with the standardisation this data got
    // (scaleX is 1 where the columns were not scaled, scaleY 1 where nothing was), rounded inwards; factors and bounds to the device;
    // lambda_0 from X'y on the host (box_host.h; no bounds, u = 1: device_absmax's value to the bit)
    float box_plan_lambda0() {
        std::vector<float> lo(p), hi(p), h(p);
        for (int j = 0; j < p; ++j) {
            lo[j] = box_round_lower(box_to_std(pb.box_lower[j], (double)d.scaleX[j], (double)d.scaleY));
            hi[j] = box_round_upper(box_to_std(pb.box_upper[j], (double)d.scaleX[j], (double)d.scaleY));
        }
        clamp.set(pb.box_lower, pb.box_upper);
        bpf.alloc((size_t)p); blo.alloc((size_t)p); bhi.alloc((size_t)p);
        ADMM_HIP_CHECK(hipMemcpyAsync(bpf.get(), pb.penalty_factor.data(), (size_t)p * sizeof(double), hipMemcpyHostToDevice, st));
        ADMM_HIP_CHECK(hipMemcpyAsync(blo.get(), lo.data(), (size_t)p * sizeof(float), hipMemcpyHostToDevice, st));
        ADMM_HIP_CHECK(hipMemcpyAsync(bhi.get(), hi.data(), (size_t)p * sizeof(float), hipMemcpyHostToDevice, st));
        read_back(h.data(), XY.get(), (size_t)p * sizeof(float), st);      // (synchronises: the host vectors may go out of scope)
        bq.pf = bpf.get(); bq.lo = blo.get(); bq.hi = bhi.get();
        return box_lambda0(h.data(), p, lo.data(), hi.data(), pb.penalty_factor.data());
    }

    // lambda_0 of the multi-task lasso: the largest ||(X'Y)_j.||_2 / w_j over the penalised rows, the norm in double from the float X'Y,
    // rounded to float (m = 1, weight 1: exactly device_absmax)
    float mt_lambda0() {
        std::vector<float> h((size_t)mt * ldp);
        read_back(h.data(), XY.get(), h.size() * sizeof(float), st);
        double best = 0.0;
        for (int j = 0; j < p; ++j) {
            if (!(pb.row_weight[j] > 0)) continue;
            double s2 = 0.0;
            for (int k = 0; k < mt; ++k) { const double v = (double)h[(size_t)k * ldp + j]; s2 += v * v; }
            best = std::max(best, std::sqrt(s2) / pb.row_weight[j]);
        }
        return (float)best;
    }
    // floats of the multi-task partial planes, 2 m (nrb + nax_rows) ldo, bounded from the shape alone (the schedule is chosen later; its
    // narrowest segments are 32 columns, so no strip has more than p32 / 32 of them)
    double mt_partial_floats() const {
        const double nrb = (double)((p + kSyRB - 1) / kSyRB), ldo = nrb * kSyRB;
        return 2.0 * mt * (nrb + (double)((p + 31) / 32)) * ldo;
    }

    // lambda_0 of the group lasso: the largest ||(X'y)_g||_2 / w_g over the penalised groups, the norm in double from the float X'y,
    // rounded to float like the Lasso's `Scalar lambda0` (singleton groups of weight 1: exactly device_absmax)
    float group_lambda0() {
        std::vector<float> h(p);
        read_back(h.data(), XY.get(), (size_t)p * sizeof(float), st);
        double best = 0.0;
        for (size_t g = 0; g + 1 < pb.group_start.size(); ++g) {
            if (!(pb.group_weight[g] > 0)) continue;
            double s2 = 0.0;
            for (int j = pb.group_start[g]; j < pb.group_start[g + 1]; ++j) s2 += (double)h[j] * (double)h[j];
            best = std::max(best, std::sqrt(s2) / pb.group_weight[g]);
        }
        return (float)best;
    }

    // ... of the sparse-group lasso: the largest lambda_g over the groups, lambda_g the smallest lambda whose two-level prox empties
    // group g started from X'y (sgl_host.h; alpha = 0: group_lambda0's value, alpha = 1 with unit weights: device_absmax's)
    float sgl_plan_lambda0() {
        std::vector<float> h(p);
        read_back(h.data(), XY.get(), (size_t)p * sizeof(float), st);
        return sgl_lambda0(h.data(), pb.group_start, pb.l1_weight, pb.group_weight);
    }

    // Whole groups into tiles for tall_group_tail_kernel: consecutive groups while they total at most kTailElems coordinates; a
    // larger group alone.  Returns the number of tiles (workgroups of the tail).
    // A sparse-group call in which NO group carries a block weight (alpha = 1, or every w_g = 0) has no block structure left: shrink is
    // exactly 1 in every group, so each column is a one-column group of weight l1_j to the bit, and it is packed as such -- the Lasso
    // with penalty factors on the Lasso tail's own tiles (32 consecutive coordinates, hence its norm partials and its decision trace
    // byte for byte), without the norms and without a multi-pass workgroup for a large group.  As soon as one group has a block weight
    // the groups are packed as admm_hip_grplasso packs them, zero-weight groups included.
    int pack_group_tiles() {
        std::vector<int2> tiles;
        std::vector<GroupCoord> coord(p);
        const bool flat = sgl && std::none_of(pb.group_weight.begin(), pb.group_weight.end(), [](double w) { return w > 0; });
        std::vector<int> each;
        if (flat) for (int j = 0; j <= p; ++j) each.push_back(j);
        const std::vector<int>& start = flat ? each : pb.group_start;
        int first = 0, count = 0;
        const auto flush = [&] { if (count > 0) tiles.push_back(make_int2(first, count)); first += count; count = 0; };
        for (size_t g = 0; g + 1 < start.size(); ++g) {
            const int gs = start[g], gn = start[g + 1] - gs;
            const double wg = flat ? 0.0 : pb.group_weight[g];
            ADMM_REQUIRE(gn >= 1 && gn <= kGroupMax && gs == first + count, "internal: bad group partition");
            for (int j = gs; j < gs + gn; ++j)
                coord[j] = GroupCoord{gs, gn, sgl && gn == 1 ? sgl_single_weight(pb.l1_weight[j], wg) : wg};
            if (count + gn > kTailElems) flush();
            count += gn;
            if (gn > kTailElems) flush();
        }
        flush();
        gtiles.alloc(tiles.size()); gcoord.alloc(coord.size());
        ADMM_HIP_CHECK(hipMemcpyAsync(gtiles.get(), tiles.data(), tiles.size() * sizeof(int2), hipMemcpyHostToDevice, st));
        ADMM_HIP_CHECK(hipMemcpyAsync(gcoord.get(), coord.data(), coord.size() * sizeof(GroupCoord), hipMemcpyHostToDevice, st));
        if (sgl) {
            gl1.alloc((size_t)p);
            ADMM_HIP_CHECK(hipMemcpyAsync(gl1.get(), pb.l1_weight.data(), (size_t)p * sizeof(double), hipMemcpyHostToDevice, st));
        }
        comm_stream_sync(st);                           // (the host vectors go out of scope)
        gq.tiles = gtiles.get(); gq.coord = gcoord.get(); gq.l1 = sgl ? gl1.get() : nullptr;
        return (int)tiles.size();
    }

    Records records() override { return {st, 5ll * p * std::max(mt, 1), &q.trace, &q.trace_cap, &q.state, &q.state_cap}; }      // multi-task: [5][m][p]

    void read_system(float* out, long long ld) override {
        if (!refine) throw Error(ADMM_ERR_INVALID_ARG, "the system matrix is only kept with ADMM_HIP_REFINE=1");
        ADMM_REQUIRE(out != nullptr && ld >= p, "bad output for the system matrix");
        ADMM_HIP_CHECK(hipMemcpy2D(out, (size_t)ld * sizeof(float), Mg.get(), (size_t)ldp * sizeof(float), (size_t)p * sizeof(float), (size_t)p, hipMemcpyDeviceToHost));
    }

    // One warm-started lambda path from a cold start (init at the first lambda, init_warm after).
    void run(LassoResult& res) override {
        admm_stats S = setup_stats;
        S.xupdate_variant = shard ? 2 : (use_sym ? 1 : 0);
        S.exchange_variant = exchange_code;
        S.refine = refine ? 1 : 0;
        S.factor_flops = dist_flops;
        res.lambda = lam_user;
        beta.zero(st); niter.zero(st);
        q.run_tag = ++run_no << kVerdictShift;          // `total` restarts at 0 below: the words an earlier run left must not match this one's
        const int init_n = std::max(p, 2 * nwg * (8 + kGateCols));
        for (int k = 0; k < std::max(mt, 1); ++k) {      // multi-task: plane by plane (every launch writes the same control block and norm partials)
            TallParams qk = q;
            if (mt) {
                const size_t o = (size_t)k * ldv;
                qk.x += o; qk.z0 += o; qk.z1 += o; qk.y0 += o; qk.y1 += o; qk.adj_z += o; qk.adj_y += o;
                qk.XY += (size_t)k * ldp; qk.u = uw.get() + (size_t)(2 * k) * ldv; qk.w = uw.get() + (size_t)(2 * k + 1) * ldv;
            }
            hipLaunchKernelGGL(tall_init_kernel, dim3((init_n + 255) / 256), dim3(256), 0, st, qk, rho, lam_int[0]);
        }
        if (q.state != nullptr && mt)      // record 0 of the iterate dump: X'Y, [m][p], in the x slot
            ADMM_HIP_CHECK(hipMemcpy2DAsync(q.state, (size_t)p * sizeof(float), XY.get(), (size_t)ldp * sizeof(float), (size_t)p * sizeof(float),
                                            (size_t)mt, hipMemcpyDeviceToDevice, st));
        else if (q.state != nullptr)      // record 0 of the iterate dump (the cold start has no iterates): X'y as this solver holds it, in the x slot
            ADMM_HIP_CHECK(hipMemcpyAsync(q.state, XY.get(), (size_t)p * sizeof(float), hipMemcpyDeviceToDevice, st));
        *hflag.p = 0;
#ifdef ADMM_HIP_PROBE
        sy.probe_idx = 0;
#endif

        const int batch = batch_iters(pb.batch_iters, 32);
        const int stride = pb.profile_stride;                          // sample every stride-th x-update with events
        size_t nev = 0;                                                // events of ev_pool used by this run
        // Single rank: no copy per poll, the deciding workgroup sets the pinned flag itself when the path has finished.
        // Sharded over ranks: every rank must enqueue the SAME number of exchanges, so the stop decision has to be a
        // deterministic function of the stream position -- the `done` word of the control block sampled in stream order after
        // each batch -- not of when a flag store happens to become visible to this host.  (No batch growth on this path.)
        const auto done_at = [&](long long g) -> const int* { return &ctl.get()[(int)(g & 1)].done; };
        const LoopTimes lt = run_until_done(st, done_at, batch, (long long)nlam * ((long long)pb.opts.maxit + 2) + 4, [&](long long g) {
            const int par = (int)(g & 1);
            const bool sample = stride > 0 && (g % stride) == stride / 2 && nev < 8192;      // mid-batch: not the launch right behind the poll event
            hipEvent_t e0 = nullptr, e1 = nullptr;
            if (sample) {
                while (ev_pool.size() < nev + 2) {
                    hipEvent_t e; ADMM_HIP_CHECK(hipEventCreate(&e));
                    ev_pool.push_back(e);
                }
                e0 = ev_pool[nev]; e1 = ev_pool[nev + 1];
                nev += 2;
            }
            // sampled launches carry start/stop events that time exactly the x-update kernel on this stream
            // the decision of this iteration rides along as one extra workgroup of the x-update launch
            const TallDecideExtra dec{q, par};
            // launch g rides the decision that leaves g + 1 taken: its tiles leave on exactly that word with the discard bit set
            SymvVerdict vd;
            if (verdict_on && !decide_first) { vd.words = verdict.get(); vd.discard = tall_verdict_word(q.run_tag, (int)(g + 1), true); vd.early = verdict.get() + kVerdictWords; vd.mid = verdict_mid; }
            const int* skip = &ctl.get()[par].done;
            // single device, one stream of the inverse: the x-update with the decision riding on it, in the form p selected
            const auto xupdate = [&] {
                if (decide_first) {
                    const TallGate gate{ctl.get() + par, P.get() + tall_norm_compact(nwg, par), nwg, q.maxit, q.nlam};
                    if (packed) symv_launch_one_packed(sy, pk, u.get(), w.get(), skip, st, gate, q.early, dec, e0, e1);
                    else sy.launch_one(M.get(), ldp, u.get(), w.get(), skip, st, gate, q.early, dec, e0, e1);
                }
                else if (use_sym) sy.launch(M.get(), ldp, u.get(), w.get(), skip, st, dec, e0, e1, vd);
                else launch_gemv_t<float, 2, 4, TallDecideExtra>(pl, M.get(), ldp, p, p, u.get(), w.get(), a_part.get(), b_part.get(), ldp, skip, st, dec, e0, e1);
            };
            const auto group_tail = [&] {
                void (*tail)(TallParams, int, GroupTailParams) =
                    decide_first ? (sgl ? tall_group_tail_kernel<TAIL_SYMV1, true> : tall_group_tail_kernel<TAIL_SYMV1>)
                    : use_sym ? (sgl ? tall_group_tail_kernel<TAIL_SYMV, true> : tall_group_tail_kernel<TAIL_SYMV>)
                            : (sgl ? tall_group_tail_kernel<TAIL_GEMV, true> : tall_group_tail_kernel<TAIL_GEMV>);
                hipLaunchKernelGGL(tail, dim3(nwg), dim3(kTailThreads), 0, st, q, par, gq);
            };
            if (mt) {
                // ceil(2m / NR) passes over the triangle, NR right-hand sides each (the decision rides on the first), then the row tail
                const int nvec = 2 * mt;
                for (int r0 = 0; r0 < nvec; r0 += mt_rhs) {
                    SymvNArgs a;
                    a.A = M.get(); a.lda = ldp; a.p = p;
                    a.v = uw.get() + (size_t)r0 * ldv; a.vstride = ldv;
                    a.dot = mdot.get() + (size_t)r0 * mq.dot_stride; a.dot_stride = mq.dot_stride;
                    a.axp = maxp.get() + (size_t)r0 * mq.axp_stride; a.axp_stride = mq.axp_stride;
                    a.nvec = std::min(mt_rhs, nvec - r0); a.ldo = sy.ldo; a.tiles = sy.tiles.get(); a.skip = skip;
                    // a sampled iteration is timed from the start of its first pass to the end of its last
                    hipEvent_t es = r0 == 0 ? e0 : nullptr, ee = r0 + mt_rhs >= nvec ? e1 : nullptr;
                    if (r0 == 0) symvn_launch(sy, mt_rhs, a, st, dec, es, ee);
                    else symvn_launch(sy, mt_rhs, a, st, SymvNoExtra(), es, ee);
                }
                hipLaunchKernelGGL(tall_mt_tail_kernel, dim3(nwg), dim3(kTailThreads), 0, st, q, par, mq);
            } else if (grouped) {                      // two launches, as the Lasso
                xupdate();
                group_tail();
            } else if (shard && peer_fused) {
                // this rank's tiles -> its share of (a, b) written into every rank's exchange slot by the reduction
                // launch itself -> the (replicated) tail waits for the K flags and sums the K slots: three launches,
                // none of them the exchange layer's
                sy.launch(M.get(), ldp, u.get(), w.get(), skip, st, dec, e0, e1);
                const PeerExchange ex = comm_peer_begin((size_t)2 * ldp * sizeof(float));
                if (peer_one) {
                    hipLaunchKernelGGL(tall_tail_kernel<TAIL_PEER1>, dim3(nwg), dim3(kTailThreads), 0, st, q, par, ex);
                } else {
                    hipLaunchKernelGGL(tall_shard_push_kernel, dim3(nwg), dim3(kTailThreads), 0, st, q, ex, ldp, skip);
                    hipLaunchKernelGGL(tall_tail_kernel<TAIL_PEER>, dim3(nwg), dim3(kTailThreads), 0, st, q, par, ex);
                }
            } else if (shard) {
                // this rank's tiles -> its share of (a, b) -> ONE all-reduce of 2 ldp floats -> the (replicated) tail
                sy.launch(M.get(), ldp, u.get(), w.get(), skip, st, dec, e0, e1);
                hipLaunchKernelGGL(tall_shard_reduce_kernel, dim3(nwg), dim3(kTailThreads), 0, st, q, ab.get(), ldp, skip);
                allreduce_sum_f32(ab.get(), (size_t)2 * ldp, st);
                hipLaunchKernelGGL(tall_tail_kernel<TAIL_GEMV>, dim3(nwg), dim3(kTailThreads), 0, st, q, par, PeerExchange{});
            } else if (use_sym && refine) {
                // x1 = Minv rhs (both candidates) -> vectors; r = rhs - M x1 in double; correction Minv r -> partials; the tail adds
                sy.launch(M.get(), ldp, u.get(), w.get(), skip, st, dec, e0, e1);
                hipLaunchKernelGGL(tall_shard_reduce_kernel, dim3(nwg), dim3(kTailThreads), 0, st, q, rab.get(), ldv, skip);
                SymvArgsD ad;
                ad.A = Mg.get(); ad.lda = ldp; ad.p = p; ad.v0 = rab.get(); ad.v1 = rab.get() + ldv;
                ad.dot0 = dD0.get(); ad.dot1 = dD1.get(); ad.axp0 = xD0.get(); ad.axp1 = xD1.get(); ad.ldo = sy.ldo; ad.tiles = sy.tiles.get(); ad.skip = skip;
                hipLaunchKernelGGL(symv2_lower_f64acc_kernel, dim3(sy.ntiles), dim3(kSyThreads), 0, st, ad);
                hipLaunchKernelGGL(tall_refine_resid_kernel, dim3(nwg), dim3(kTailThreads), 0, st, q, dD0.get(), dD1.get(), xD0.get(), xD1.get(),
                                   ruw.get(), ruw.get() + ldv, skip);
                sy.launch(M.get(), ldp, ruw.get(), ruw.get() + ldv, skip, st, SymvNoExtra());
                hipLaunchKernelGGL(tall_tail_kernel<TAIL_SYMV>, dim3(nwg), dim3(kTailThreads), 0, st, q, par, PeerExchange{});
            } else if (box) {                          // two launches, as the Lasso
                xupdate();
                if (decide_first) hipLaunchKernelGGL(tall_box_tail_kernel<TAIL_SYMV1>, dim3(nwg), dim3(kTailThreads), 0, st, q, par, bq);
                else if (use_sym) hipLaunchKernelGGL(tall_box_tail_kernel<TAIL_SYMV>, dim3(nwg), dim3(kTailThreads), 0, st, q, par, bq);
                else hipLaunchKernelGGL(tall_box_tail_kernel<TAIL_GEMV>, dim3(nwg), dim3(kTailThreads), 0, st, q, par, bq);
            } else {
                xupdate();
                if (decide_first) hipLaunchKernelGGL(tall_tail_kernel<TAIL_SYMV1>, dim3(nwg), dim3(kTailThreads), 0, st, q, par, PeerExchange{});
                else if (use_sym) hipLaunchKernelGGL(tall_tail_kernel<TAIL_SYMV>, dim3(nwg), dim3(kTailThreads), 0, st, q, par, PeerExchange{});
                else hipLaunchKernelGGL(tall_tail_kernel<TAIL_GEMV>, dim3(nwg), dim3(kTailThreads), 0, st, q, par, PeerExchange{});
            }
        }, LoopOpts{shard ? nullptr : hflag.p, 0, false});
        S.t_loop = lt.wall_s; S.loop_ms_events = lt.events_ms; S.xupdate_launches = lt.launched;
        const CtlPair<TallCtl> hctl = read_ctl(ctl.get());      // both slots: decisions taken
        unsigned long long early = 0;
        if (verdict_on) {                                      // the two-vector kernel counts in slot 0, the one-vector kernel in all of them
            std::vector<unsigned long long> slots((size_t)kSyEarlySlots * kSyVerdictStride);
            ADMM_HIP_CHECK(hipMemcpy(slots.data(), verdict.get() + kVerdictWords, slots.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
            for (int k = 0; k < kSyEarlySlots; ++k) early += slots[(size_t)k * kSyVerdictStride];
        }
        t_early_exits = (long long)early;
        WIDE_PROBE_DUMP(probe);
        if (nev > 0) {
            double tot = 0;
            for (size_t k = 0; k + 1 < nev; k += 2) {
                float m1 = 0.f;
                ADMM_HIP_CHECK(hipEventElapsedTime(&m1, ev_pool[k], ev_pool[k + 1]));
                tot += m1;
            }
            S.xupdate_samples = (long long)(nev / 2);
            S.xupdate_ms_avg = tot / (double)(nev / 2);
        }

        // ---- results: niter, beta on the original scale (DataStd::recover, Lasso.cpp:108-111)
        ADMM_HIP_CHECK(hipMemcpyAsync(hbeta, beta.get(), (size_t)nlam * p * std::max(mt, 1) * sizeof(float), hipMemcpyDeviceToHost, st));
        comm_stream_sync(st);
        if (mt) {      // per response, with that response's mean: coefficients [nlam][m][p + 1]; niter is one count per lambda
            const size_t col = (size_t)p + 1;
            std::vector<float> bk;
            res.beta.assign(col * mt * nlam, 0.f);
            for (int k = 0; k < mt; ++k) {
                S.total_iter = read_out_path<float>(d, hbeta + (size_t)k * p, nlam, niter.get(), col, 0, res.niter, bk, INT_MAX, (size_t)mt * p, &d.meanYs[k]);
                for (int l = 0; l < nlam; ++l) std::memcpy(res.beta.data() + ((size_t)l * mt + k) * col, bk.data() + (size_t)l * col, col * sizeof(float));
            }
        } else {
            S.total_iter = read_out_path<float>(d, hbeta, nlam, niter.get(), (size_t)p + 1, 0, res.niter, res.beta, INT_MAX, 0, nullptr, &clamp);
        }
        decisions = hctl.c[0].done ? hctl.total() : 0;      // (the sticky no-op decisions after `done` do not write)
        res.stats = S;
    }
};

std::unique_ptr<LassoPlan> make_tall_plan(DeviceData<float>&& d, const LassoProblem& pb, hipStream_t st) {
    return std::unique_ptr<LassoPlan>(new TallPlan(std::move(d), pb, st));
}

}  // namespace admm
