// Least-absolute-deviation and basis-pursuit solvers (fp64), device resident.
//
// Replaces ADMMLAD / ADMMBP driven by FADMMBase::solve:
//   /root/reference/src/FADMMBase.h:109-133 (update_rho), :185-265 (solve)
//   /root/reference/src/ADMMLAD.h:62-107 (next_x/next_z/next_residual), :152-169 (eps/resid), :172-225 (setup, get_x)
//   /root/reference/src/ADMMBP.h:48-93, :138-153, :157-197
//
// Per iteration: `head` (decision of the previous iteration evaluated redundantly by every
// workgroup from the norm partials -> acceleration/restart scalars, rho adaptation, convergence;
// then adj_z/adj_y and the vector the projection is applied to), 2-3 streaming mat-vecs
// (gemv_t on the matrix and on its stored transpose, so every product reads contiguous columns),
// `tail` (x, soft-threshold z, dual y, six squared norms).  The host enqueues iterations in
// batches and polls a sticky `done` word; no per-iteration synchronisation.
#include "prep.h"
#include "gemv_kernels.h"
#include "gather_kernels.h"
#include "solvers.h"
#include "test_hooks.h"
#include <cstring>
#include <cstdio>
#include <type_traits>
#include "loop_driver.h"

namespace admm {

struct DenseCtl {
    double rho, eps_primal, eps_dual, adj_a, adj_c, tau;
    int restart, iter, done, first, total, niter, conv, pad;
};

struct DenseParams {
    int dim, prob, maxit, nwg_tail;          // prob: 0 = LAD, 1 = BP
    double eps_abs, eps_rel, sqrt_dim, extra_norm;
    const double* data_vec;                   // LAD: y (n);  BP: A'(AA')^-1 b (p)
    double *x, *z0, *z1, *y0, *y1, *adj_z, *adj_y, *vec;
    const double* gout; int gout_nseg; long long gout_stride;
    DenseCtl* ctl;                            // [2]
    double* P;                                // [nwg_tail][8]
    int* done;
    double* trace; long long trace_cap;       // optional decision records (admm_hip_lad_traced / admm_hip_bp_traced), or NULL
    double* state; long long state_cap;       // optional [state_cap][5][dim] iterates x, z, y, adj_z, adj_y of every iteration (admm_hip_lad_state / admm_hip_bp_state), or NULL
    // BP, one-pass form (round 5; bpn = 0: the two-pass form).  B = L^-1 A has B B' = I, so B x = B vec + B A'(AA')^-1 b - B B' B vec
    // = L^-1 b =: w0 for EVERY iterate; with y = adj_y + rho (x - z) the n-vector B y follows from B adj_y and B z, B adj_z / B adj_y
    // from the same accelerate / restart combinations as adj_z / adj_y, and w = B vec = B adj_z - B adj_y / rho needs no pass over B:
    // only B z (z = prox output, sparse: gather_kernels.h) and the one streaming product B'w remain.
    // The recurrence is dead-beat, not an integrator: if the held B adj_y is off by e, w is off by -e / rho, then B x is off by
    // -e / rho as well and the true B y_new = B adj_y + e + rho (w0 - e / rho - B z_new) equals the held one.  What is left per iteration
    // is (I - B B') B vec, i.e. the rounding of the factorisation, and the rounding of the elementwise updates.
    int bpn;
    // (w0 is BP's; sgn is the signed logit prox's, kProxLogitS: the signs of the label column the loop fits, or, in the slotted loop, the
    // sign matrix.  A LAD-type loop has bpn = 0 and never reads w0, so the two share one word and the argument block of every kernel keeps
    // its size and offsets.)
    union { const double* w0; const double* sgn; };
    double *Bz0, *Bz1, *By0, *By1, *Badjy, *w;
    const double* gpart; int gngroups; long long gpstride;
    // LAD, one-pass form (round 6; lp = 0: the two-pass form).  The projection needs X'vec with vec = d - adj_y / rho + adj_z, and adj_z /
    // adj_y are the accelerate / restart combinations of the two latest z / y: X'vec is the same combination of the p-vectors X'd
    // (fixed), X'z and X'y of the two latest iterates -- and X'z_new, X'y_new can be formed by the launch that produces z_new, y_new:
    // lad_rows_kernel streams the ROWS of X once, forms x_i = row_i . s, the prox and the dual for that row, and adds row_i z_i,
    // row_i y_i to its partials of X'z, X'y.  One pass over X per iteration instead of two (X'vec, then X s); the p-vectors are direct
    // products of the current iterates, not recurrences: nothing accumulates.
    int lp;
    int sgn_cols;                             // kProxLogitE, slotted loop: the label columns of the sign matrix -- fit k reads column k mod sgn_cols (in the padding behind lp: the argument block keeps its size and offsets)
    const double* Xd;                         // X'd [lp]
    double *Xz0, *Xz1, *Xy0, *Xy1;            // X'z, X'y in the slots of z0 / z1, y0 / y1
    double* u;                                // X'vec of this iteration
    const double* cpart; int cnwg; long long cstride;      // the rows launch's partials: [cnwg][2][cstride] (X'z_new | X'y_new)
    // the prox of g(z) = 2 sum rho_tau(-z_i) (quantile regression, admm_hip_quantreg): thresholds c_hi / rho above, c_lo / rho below,
    // c_hi = 2 (1 - tau), c_lo = 2 tau.  LAD (tau = 0.5) and BP: both 1.0 -- the symmetric soft-threshold with 1 / rho.
    double c_hi, c_lo;
};

constexpr int kDenseThreads = 256;

__device__ __forceinline__ double soft2(double v, double hi, double lo) {
    return v > hi ? v - hi : (v < -lo ? v + lo : 0.0);
}
// The prox of g(z) = sum w(z_i) H_delta(z_i) / rho, w = c_hi above zero and c_lo below, H_delta the Huber function (r^2 / 2 up to
// |r| = delta, linear beyond), with hi = c_hi / rho, lo = c_lo / rho:
//     v >  delta (1 + hi): v - delta hi     v < -delta (1 + lo): v + delta lo     between: v / (1 + hi) for v >= 0, v / (1 + lo) below
// (tests/huber_oracle.py restates these four lines).  Formed here on |v| with the side's constant chosen first: one division, and
// bit for bit the same, since v beyond a knee has that knee's sign (delta > 0) and negation commutes with every rounding.
// delta = +inf: the knee is +inf and only the central branch is taken.  Every operation is rounded on its own.  The side's constant
// is made opaque so that the derived constants (1 + pen, delta (1 + pen), delta pen: two of each) are formed per element and not
// held in registers across the rows loop -- there they cost the slotted kernels a slot.
__device__ __forceinline__ double huber2(double v, double hi, double lo, double delta) {
#pragma clang fp contract(off)
    double pen = v >= 0.0 ? hi : lo;
    asm volatile("" : "+v"(pen));
    const double a = fabs(v), onep = 1.0 + pen;
    const double z = a > delta * onep ? a - delta * pen : a / onep;
    return copysign(z, v);
}
// The z-update's prox, chosen at compile time: the kernels below take PROX as a template parameter and the knee (admm_hip_huber: delta
// in the units of the standardised response, +inf = expectile regression) as their LAST argument, behind everything the soft-threshold
// instantiations (LAD, BP, quantile regression) read: those neither hold nor load it and keep their registers and instruction counts
// (profiles/huber_loss.md).
constexpr int kProxSoft = 0, kProxHuber = 1, kProxLogit = 2, kProxLogitS = 3, kProxLogitR = 4, kProxLogitE = 5, kProxPoisE = 6;
// kProxLogitS (admm_hip_logit_multi): the same loss on the UNFOLDED matrix [X | 1], the label's sign taken inside the prox --
// prox of log(1 + e^(-s z)) / rho at v is s logit2(s v, t).  Multiplying by +-1 is exact and rounding is symmetric in sign, so every n-vector
// of this loop is s times the folded loop's and every p-vector, norm and decision equal to it: the matrix no longer depends on the labels.
// kProxLogitR (admm_hip_logit_ridge): kProxLogitS on the matrix with the ridge rows sqrt(lambda) e_j' appended.  Their entries of the sign
// vector are 0.0 (the padding logit_sign_matrix_kernel writes anyway), and sign 0 means a square-loss row: the prox of z^2 / (2 rho) at v,
// z = v (rho / (1 + rho)) -- in this association, rounded operation by operation (tests/logit_ridge_oracle.py replays it).  The rows with
// sign +-1 run the S form's expressions.
// kProxLogitE (admm_hip_logit_enet): kProxLogitS on the matrix with the penalty rows c e_j' appended (c^2 = the number of data rows, for
// every lambda and alpha: the penalty's constants sit in the prox, not in the row).  A row of sign 0.0 takes the elastic net's prox with
// the fit's constants c_hi = lambda alpha / c, c_lo = lambda (1 - alpha) / c^2: enet2 below.  The rows with sign +-1 run the S form's
// expressions (t = 1 / rho whatever c_hi is).
// kProxPoisE (admm_hip_poisson): kProxLogitE's matrix and penalty rows with the Poisson loss e^z - y z on the data rows.  The "sign" matrix
// carries the row's COUNT y_i >= 0 instead of +-1 and the marker -1.0 on every penalty row and padding entry (counts are refused below
// zero): an entry >= 0 takes pois2(v, y, 1 / rho) below -- no sign round trip --, a marker row enet2 as the E form calls it.
// What the kernels and the host need to know of a kind, stated once and indexed by it.  iterative: the prox is a Newton iteration and
// is formed once per row by the rows kernels' prox lanes; tagged: the per-row entry of DenseParams::sgn (sign or count) travels in the
// response's place and row_prox_tagged below holds the case analysis; enet: penalty rows whose constants are the fit's c_hi / c_lo.
// auto_slots: what QUANT_SLOTS=0 picks on the one-pass branch.  max_slots[NPT - 1], NPT = 1 .. 6 the columns a thread of the rows
// kernels holds per row (lad_npt): how many slots the registers of quant_rows_kernel hold -- the instantiations without scratch
// (tests/test_lad_kernels_asm.py pins that they have none); 1 = no slotted form.  The dispatch below instantiates
// quant_rows_kernel<NPT, S, kind> for S = 2 .. max_slots[NPT - 1] and nothing else.
struct ProxKind {
    bool iterative, tagged, enet;
    int auto_slots;
    int max_slots[6];
};
constexpr int kProxKindCount = 7, kLadMaxNpt = 6;
constexpr ProxKind kProxKinds[kProxKindCount] = {
    // kProxSoft (admm_hip_quantreg).  auto 1: DESIGN §8, decided by scripts/bench_quantreg.py.  NPT 6 is six double2 per row: two slots would spill
    {false, false, false, 1, {4, 4, 4, 3, 2, 1}},
    // kProxHuber (admm_hip_huber).  auto: as many as the layout admits (measured: scripts/bench_huber.py, profiles/huber_loss.md).
    // (4, 3) spills 16 bytes and fell away
    {false, false, false, 4, {4, 4, 4, 2, 2, 1}},
    // kProxLogit (admm_hip_logit): the matrix carries the labels, one fit per call -- no slotted form
    {true, false, false, 1, {1, 1, 1, 1, 1, 1}},
    // kProxLogitS (admm_hip_logit_multi).  auto: as many as the layout admits (measured: scripts/bench_logit_multi.py,
    // profiles/logit_multi.md).  (4, 3) spills 64 bytes, (5, 2) 24 (profiles/logit_multi.md)
    {true, true, false, 4, {4, 4, 4, 2, 1, 1}},
    // kProxLogitR (admm_hip_logit_ridge).  auto: ahead of serial at every layout with slots (measured: scripts/bench_logit_ridge.py,
    // profiles/logit_ridge.md).  The S form's table (profiles/logit_ridge.md)
    {true, true, false, 4, {4, 4, 4, 2, 1, 1}},
    // kProxLogitE (admm_hip_logit_enet).  auto: ahead of serial at every layout with slots (measured: scripts/bench_logit_enet.py,
    // profiles/logit_enet.md).  The R form's table less (3, 4), which spills 16 bytes (profiles/logit_enet.md)
    {true, true, true, 4, {4, 4, 3, 2, 1, 1}},
    // kProxPoisE (admm_hip_poisson).  auto: ahead of serial at every layout with slots (measured: scripts/bench_poisson.py,
    // profiles/poisson.md).  The kProxPoisE instantiations without scratch (profiles/poisson.md)
    {true, true, true, 4, {4, 4, 3, 2, 1, 1}},
};
// The prox of (c_hi |z| + c_lo z^2 / 2) / rho at v: t = c_hi / rho, d = 1 + c_lo / rho, z = soft(v, t) / d -- in this association, every
// operation rounded on its own (tests/logit_enet_oracle.py replays it)
__device__ __forceinline__ double enet2(double v, double c_hi, double c_lo, double rho) {
#pragma clang fp contract(off)
    const double t = c_hi / rho, d = 1.0 + c_lo / rho;
    return soft2(v, t, t) / d;
}
// The prox of g(z) = log(1 + e^-z) / rho (admm_hip_logit: the binomial negative log-likelihood on the sign-folded matrix), t = 1 / rho:
// the root of h(z) = z - v - t sigma(-z), sigma(-z) = 1 / (1 + e^z), by Newton's iteration.  h is increasing, 1 <= h' <= 1 + t / 4, convex
// left of zero and concave right of it, the root lies in [v, v + t]; from the start below (v when v > 0, v + t when v + t < 0, else 0)
// the double iteration approaches it from one side, every step clamped to the bracket.  sigma(-z) is formed from e = exp(-|z|) -- e / (1 + e)
// for z >= 0, 1 / (1 + e) below -- so nothing overflows for any finite v.  Every operation is rounded on its own: the result is ONE
// function of (v, t) wherever it is called (tail and rows kernels, test hook), whichever lanes run beside it.
// Cost (profiles/logit_loss.md): two Newton steps in float (__expf) from the same start, inside the same clamp, seed the double
// iteration -- at t <= 1, where the double iteration alone takes five steps, about three are left.  It stops on the step,
// |z_new - z| <= 2^-50 max(1, |z|, |v|) (h is evaluated to a few ulp of max(|z|, |v|): t sigma = z - v at the root), under a cap of
// kLogitMaxSteps.  The steps before the quadratic phase grow like ln t -- without the seed 10 at t = 1e3, 12 at 1e4, 16 at 1e6, 29 at
// 1e12 (tests/logit_oracle.py's prox) --, which the cap leaves room for: no rho the loop's adaptation can reach is refused.  |v| or t
// beyond 1e30 skip the float seed (it would overflow).
constexpr int kLogitMaxSteps = 64;
__device__ __forceinline__ double logit2(double v, double t) {
#pragma clang fp contract(off)
    const double hi = v + t;
    double z = v > 0.0 ? v : (hi < 0.0 ? hi : 0.0);
    if (fabs(v) < 1e30 && t < 1e30) {
        const float vf = (float)v, tf = (float)t, hf = vf + tf;
        float zf = (float)z;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const float e = __expf(-fabsf(zf));
            const float s = (zf >= 0.f ? e : 1.f) / (1.f + e);
            const float h = zf - vf - tf * s, d = 1.f + tf * s * (1.f - s);
            zf = fminf(fmaxf(zf - h / d, vf), hf);
        }
        z = fmin(fmax((double)zf, v), hi);
    }
    for (int k = 0; k < kLogitMaxSteps; ++k) {
        const double e = exp(-fabs(z));
        const double s = (z >= 0.0 ? e : 1.0) / (1.0 + e);
        const double h = z - v - t * s, d = 1.0 + t * s * (1.0 - s);
        const double zn = fmin(fmax(z - h / d, v), hi);
        const double moved = fabs(zn - z);
        z = zn;
        if (moved <= 0x1p-50 * fmax(1.0, fmax(fabs(z), fabs(v)))) break;
    }
    return z;
}
// The prox of g(z) = (e^z - y z) / rho (admm_hip_poisson: the Poisson negative log-likelihood of the count y >= 0 at the linear predictor
// z), t = 1 / rho: the root of h(z) = z + t e^z - w, w = v + t y, by Newton's iteration.  h is increasing and convex, h' = 1 + t e^z >= 1,
// and the root lies at or below w; from a point right of the root Newton descends monotonically, so the start decides what exp sees.
// w >= t (h(0) <= 0: the root is >= 0): the root is also <= ln(w / t), start min(w, L) with L an upper estimate of ln(w / t); below
// that (root < 0; ln(w / t) is NOT a bound there -- started from it the iteration begins left of the root) min(w, 0).
// L: the FLOAT logarithm of the quotient (one hardware instruction; the double logarithm cost every rows kernel about 22 VGPRs, two
// of them scratch, profiles/poisson.md) plus 2^-18 (1 + ln), above its error; a quotient beyond 2^100 (or overflowed: t tiny) takes
// (ilogb(w) - ilogb(t) + 1) ln 2, which lies above ln(w / t) by less than 2 ln 2.  With these starts t e^z <= 4 max(w, t) at every
// evaluation: nothing overflows for any finite v, any y >= 0 and any t > 0.  Every step is clamped to <= w.  A start that rounding
// puts left of the root all the same takes one step to its right and descends from there (the clamp is w, not the start).  It
// stops on the step, |z_new - z| <= 2^-50 max(1, |z|, |w|), under a cap of kPoisMaxSteps.  Steps (tests/poisson_oracle.py's prox):
// 6 - 8 at t <= 1, 11 at 1e3, 17 at 1e6, 30 at 1e12 -- about one per unit of ln t before the quadratic phase.  Every operation is
// rounded on its own: ONE function of (v, y, t) wherever it is called (tail and rows kernels, test hook).
constexpr int kPoisMaxSteps = 64;
__device__ __forceinline__ double pois2(double v, double y, double t) {
#pragma clang fp contract(off)
    const double w = v + t * y;
    double z = fmin(w, 0.0);
    if (w >= t) {
        const double q = w / t;                                  // >= 1; +inf where the quotient overflows
        const double lf = (double)__logf((float)q);
        z = fmin(w, q < 0x1p100 ? lf + 0x1p-18 * (1.0 + lf) : (double)(ilogb(w) - ilogb(t) + 1) * 0.6931471805599453);
    }
    for (int k = 0; k < kPoisMaxSteps; ++k) {
        const double e = t * exp(z);
        const double h = z + e - w, d = 1.0 + e;
        const double zn = fmin(z - h / d, w);
        const double moved = fabs(zn - z);
        z = zn;
        if (moved <= 0x1p-50 * fmax(1.0, fmax(fabs(z), fabs(w)))) break;
    }
    return z;
}
template <int PROX>
__device__ __forceinline__ double prox2(double v, double hi, double lo, double delta) {
    if (PROX == kProxLogit) return logit2(v, hi);      // hi = c_hi / rho with c_hi = 1: t
    if (PROX == kProxHuber) return huber2(v, hi, lo, delta);
    return soft2(v, hi, lo);
}
// The row prox of the tagged kinds, the one statement of it (tail kernel, both rows kernels).  tag() returns the row's entry of the sign
// or count column; c_hi / c_lo are the fit's penalty constants (read by the enet kinds only).  t = 1 / rho for every kind: the S and R
// fits carry c_hi = 1.0 (LadProx's default), so the c_hi / rho the serial kernels once formed for them is the same double.  The rows
// kernels pass a callable that reads LDS on every call: the tag is read again behind the Newton iteration (the barrier below keeps the
// two reads apart), not held in registers across it.
// The enet kinds know one more tag, the HELD-OUT data row of a cross-validation fold (admm_hip_logit_enet_cv, admm_hip_poisson_cv): its
// loss is zero and the prox of the zero function is the identity, z = v.  The fold's fit on the full matrix is then the training rows'
// problem.  No call but the cross-validation's writes these two values into a tag matrix.
constexpr double kHeldOutLogitE = 2.0, kHeldOutPoisE = -2.0;
// A held-out row is no row of the fold's problem: it stays out of the norms ||x||, ||z||, ||y|| the stop thresholds are scaled by (and
// out of their sqrt(rows): LadProx::live_rows), so a fold's fit stops where the training rows' own loop would measure itself.  Its
// residuals stay in: r is zero there up to rounding and z - z_old is what the x-update moved.
template <int PROX>
__device__ __forceinline__ bool row_held_out(double tag) {
    if constexpr (PROX == kProxPoisE) return tag == kHeldOutPoisE;
    else if constexpr (PROX == kProxLogitE) return tag == kHeldOutLogitE;
    else return false;
}
template <int PROX, class TAG>
__device__ __forceinline__ double row_prox_tagged(double v, TAG tag, double c_hi, double c_lo, double rho) {
#pragma clang fp contract(off)
    if constexpr (PROX == kProxPoisE) {
        const double cnt = tag();                                    // >= 0: a data row's count; the marker -1.0: a penalty row; -2.0: held out
        if (cnt == kHeldOutPoisE) return v;
        return cnt < 0.0 ? enet2(v, c_hi, c_lo, rho) : pois2(v, cnt, 1.0 / rho);
    } else {
        if (PROX == kProxLogitR && tag() == 0.0) return v * (rho / (1.0 + rho));
        if (PROX == kProxLogitE && tag() == kHeldOutLogitE) return v;
        if (PROX == kProxLogitE && tag() == 0.0) return enet2(v, c_hi, c_lo, rho);
        const double zs = logit2(tag() * v, 1.0 / rho);              // s logit2(s v, t)
        asm volatile("" ::: "memory");
        return tag() * zs;
    }
}
// lane l's double in every lane (l uniform): two scalar reads
__device__ __forceinline__ double read_lane_f64(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// The six squared norms of the previous iteration: the tail's (rows launch's) partials summed in workgroup order.  pstage: nwg_tail * 8 doubles.
__device__ __forceinline__ void dense_head_sums(const DenseParams& q, double* pstage, double (&sums)[8]) {
    const int np = q.nwg_tail * 8;
    for (int k = threadIdx.x; k < np; k += kDenseThreads) pstage[k] = q.P[k];
    __syncthreads();
    if (threadIdx.x < 6) {
        double s = 0.0;
        for (int w = 0; w < q.nwg_tail; ++w) s += pstage[w * 8 + threadIdx.x];
        sums[threadIdx.x] = s;
    }
    __syncthreads();
}

// The decision on the previous iteration (FADMMBase.h:213-259): the control block the iteration runs with, whether the extrapolated
// pair is formed, and what the decision trace records.
struct DenseDecision {
    DenseCtl out;
    bool write_adj;
    double tr_rp, tr_rd, tr_c, tr_code;
};
__device__ __forceinline__ DenseDecision dense_decide(const DenseParams& q, const DenseCtl& in, const double* sums) {
    const double r2 = sums[0], dz2 = sums[1], daz2 = sums[2], x2 = sums[3], z2 = sums[4], y2 = sums[5];
    DenseDecision D;
    DenseCtl& out = D.out;
    out = in;
    out.first = 0;
    D.write_adj = true;
    D.tr_rp = 0; D.tr_rd = 0; D.tr_c = 0; D.tr_code = ADMM_TRACE_COLD;
    if (!in.first) {
        const double rp = sqrt(r2), rd = in.rho * sqrt(dz2);
        D.tr_rp = rp; D.tr_rd = rd;
        if (rp < in.eps_primal && rd < in.eps_dual) {          // converged(): adj_z/adj_y/rho stay as they are
            out.done = 1; out.conv = 1; out.niter = in.iter + 1;
            D.write_adj = false;
            D.tr_code = ADMM_TRACE_CONVERGED;
        } else {
            const double old_c = in.adj_c;
            const double c = in.rho * rp * rp + in.rho * daz2;
            D.tr_c = c; D.tr_code = c < 0.999 * old_c ? ADMM_TRACE_ACCELERATE : ADMM_TRACE_RESTART;
            if (c < 0.999 * old_c) {
                const double old_a = in.adj_a;
                const double a = 0.5 + 0.5 * sqrt(1.0 + 4.0 * old_a * old_a);
                out.adj_a = a; out.adj_c = c; out.tau = (old_a - 1.0) / a; out.restart = 0;
            } else {
                out.adj_a = 1.0; out.adj_c = old_c / 0.999; out.tau = -1.0; out.restart = 1;
            }
            if (in.iter > 5) {                                 // update_rho(), FADMMBase.h:109-133,258-259
                double rho = in.rho;
                if (rp / in.eps_primal > 10 * rd / in.eps_dual) rho *= 2;
                else if (rd / in.eps_dual > 10 * rp / in.eps_primal) rho /= 2;
                if (rp < in.eps_primal) rho /= 1.2;
                if (rd < in.eps_dual) rho *= 1.2;
                out.rho = rho;
            }
            out.iter = in.iter + 1;
            if (in.iter + 1 >= q.maxit) { out.done = 1; out.conv = 0; out.niter = q.maxit + 1; }
        }
    } else {
        out.tau = 0.0; out.restart = 0;
    }
    out.eps_primal = fmax(fmax(sqrt(x2), sqrt(z2)), q.extra_norm) * q.eps_rel + q.sqrt_dim * q.eps_abs;
    out.eps_dual = sqrt(y2) * q.eps_rel + q.sqrt_dim * q.eps_abs;
    out.total = out.done ? in.total : in.total + 1;
    return D;
}

// The vectors the iteration starts from: adj_z / adj_y (accelerate / restart combination of the two latest z / y), the vector the
// projection is applied to, and the same step for the one-pass forms' recurrences.  Every workgroup takes its share.
__device__ __forceinline__ void dense_head_vectors(const DenseParams& q, const DenseCtl& in, const DenseCtl& out) {
    const int cur = in.total & 1;
    const double* zc_ = cur ? q.z1 : q.z0; const double* yc_ = cur ? q.y1 : q.y0;
    const double* zo_ = cur ? q.z0 : q.z1; const double* yo_ = cur ? q.y0 : q.y1;
    const double t = out.tau, t1 = 1.0 + out.tau, rho = out.rho;
    for (int i = blockIdx.x * kDenseThreads + threadIdx.x; i < q.dim; i += gridDim.x * kDenseThreads) {
        // no fused multiply-adds in the elementwise arithmetic: the reference is built without them (lasso_tall.hip, tall_update_elem)
#pragma clang fp contract(off)
        double adjz, adjy;
        if (out.restart) { adjz = zo_[i]; adjy = yo_[i]; }
        else { adjz = t1 * zc_[i] - t * zo_[i]; adjy = t1 * yc_[i] - t * yo_[i]; }
        q.adj_z[i] = adjz; q.adj_y[i] = adjy;
        // LAD: vec = y - adj_y / rho + adj_z (ADMMLAD.h:64-65);  BP: vec = -adj_y / rho + adj_z (ADMMBP.h:50-55)
        q.vec[i] = (q.prob == 0 ? q.data_vec[i] : 0.0) - adjy / rho + adjz;
    }
    if (q.bpn > 0) {
        // the same step for the n-vectors B z, B y, B adj_z, B adj_y (see DenseParams): B z_new = the gather launch's partial rows
        // summed in group order; B y_new from the adj_y and the rho the tail used (in.rho); then w = B vec for this iteration
        double* Bzc = cur ? q.Bz1 : q.Bz0; double* Byc = cur ? q.By1 : q.By0;
        const double* Bzo = cur ? q.Bz0 : q.Bz1; const double* Byo = cur ? q.By0 : q.By1;
        for (int i = blockIdx.x * kDenseThreads + threadIdx.x; i < q.bpn; i += gridDim.x * kDenseThreads) {
#pragma clang fp contract(off)
            double bz = 0.0;
            for (int c0 = 0; c0 < q.gngroups; c0 += 8) {
                double tv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) tv[u] = q.gpart[(size_t)min(c0 + u, q.gngroups - 1) * q.gpstride + i];
#pragma unroll
                for (int u = 0; u < 8; ++u) bz += c0 + u < q.gngroups ? tv[u] : 0.0;
            }
            const double by = in.first ? 0.0 : q.Badjy[i] + in.rho * (q.w0[i] - bz);
            const double bzo = Bzo[i], byo = Byo[i];
            Bzc[i] = bz; Byc[i] = by;
            double badjz, badjy;
            if (out.restart) { badjz = bzo; badjy = byo; }
            else { badjz = t1 * bz - t * bzo; badjy = t1 * by - t * byo; }
            q.Badjy[i] = badjy;
            q.w[i] = badjz - badjy / rho;
        }
    }
    if (q.lp > 0) {
        // X'z, X'y of the iterate the rows launch has just produced (its partials summed in workgroup order) into the `cur` slots, then
        // u = X'vec as the combination the adj vectors above are of z / y
        double* Xzc = cur ? q.Xz1 : q.Xz0; double* Xyc = cur ? q.Xy1 : q.Xy0;
        const double* Xzo = cur ? q.Xz0 : q.Xz1; const double* Xyo = cur ? q.Xy0 : q.Xy1;
        // eight lanes share an element: lane `sub` adds the partial rows sub, sub + 8, ... (eight requests of each vector in flight), the eight
        // sums are added in a fixed order -- one memory round trip per 64 partial rows instead of one per 8
        const int sub = threadIdx.x & 7;
        const int epb = kDenseThreads / 8;                                // elements per block and pass
        for (int i0 = blockIdx.x * epb; i0 < q.lp; i0 += gridDim.x * epb) {
#pragma clang fp contract(off)
            const int i = min(i0 + (int)(threadIdx.x >> 3), q.lp - 1);    // (clamped: whole groups of eight lanes take part in the exchange)
            double xz = 0.0, xy = 0.0;
            for (int w0 = sub; w0 < q.cnwg; w0 += 64) {
                double tz[8], ty[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const size_t w = (size_t)min(w0 + 8 * k, q.cnwg - 1);
                    tz[k] = q.cpart[(w * 2) * q.cstride + i]; ty[k] = q.cpart[(w * 2 + 1) * q.cstride + i];
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) { xz += w0 + 8 * k < q.cnwg ? tz[k] : 0.0; xy += w0 + 8 * k < q.cnwg ? ty[k] : 0.0; }
            }
#pragma unroll
            for (int m = 1; m < 8; m <<= 1) { xz += __shfl_xor(xz, m, 64); xy += __shfl_xor(xy, m, 64); }
            if (sub != 0 || i0 + (int)(threadIdx.x >> 3) >= q.lp) continue;
            if (in.first) { xz = 0.0; xy = 0.0; }
            const double xzo = Xzo[i], xyo = Xyo[i];
            Xzc[i] = xz; Xyc[i] = xy;
            double xadjz, xadjy;
            if (out.restart) { xadjz = xzo; xadjy = xyo; }
            else { xadjz = t1 * xz - t * xzo; xadjy = t1 * xy - t * xyo; }
            q.u[i] = q.Xd[i] - xadjy / rho + xadjz;
        }
    }
}

__global__ void __launch_bounds__(kDenseThreads)
dense_head_kernel(DenseParams q, int par) {
    __shared__ double sums[8];
    extern __shared__ __attribute__((aligned(16))) double pstage[];
    const DenseCtl in = load_ctl_vector(q.ctl + par);
    DenseCtl* outp = &q.ctl[par ^ 1];
    if (in.done) {
        if (blockIdx.x == 0 && threadIdx.x == 0) *outp = in;
        return;
    }
    dense_head_sums(q, pstage, sums);
    const DenseDecision D = dense_decide(q, in, sums);
    const DenseCtl& out = D.out;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *outp = out;
        if (out.done) *q.done = 1;
        if (q.trace != nullptr && in.total < q.trace_cap) {      // what FADMMBase.h:135-170 (print_row, commented out there) would print
            double* t = q.trace + (size_t)in.total * ADMM_TRACE_FIELDS;
            t[0] = 0.0; t[1] = in.iter; t[2] = in.eps_primal; t[3] = in.eps_dual; t[4] = D.tr_rp; t[5] = D.tr_rd;
            t[6] = D.tr_c; t[7] = in.adj_c; t[8] = D.tr_code; t[9] = in.rho; t[10] = out.rho; t[11] = 0.0;
        }
    }
    if (!D.write_adj) return;
    dense_head_vectors(q, in, out);
}

// ---- the slotted loop of admm_hip_quantreg: S independent problems (the quantiles of a grid) advance in the same three launches
struct QuantGrid {
    int nslots, ntau;
    long long slot_stride;                    // doubles between two slots' vectors (see quant_slot_params)
    double rho0;                              // opts.rho: every quantile starts cold
    int* next;                                // [2] the first quantile no slot has taken yet, double-buffered like the control blocks
    int* idle;                                // [nslots] sticky: the slot has run out of quantiles (the skip word of its (X'X)^-1 u product)
    int* niter; double* rho_fin;              // [ntau] per quantile: iterations (LAD's convention) and final rho
    double* fin; long long fin_ld;            // [ntau][fin_ld] y - adj_y / rho + adj_z of the finished loop: what get_x needs
};
// kProxLogitE: the grid with one more per-fit buffer beside `fin` -- the entries [zrow0, zrow0 + zrows) (the penalty rows) of the LAST z
// of every finished fit, the prox output of its final iteration, which the elastic net returns in place of get_x's dense read-out.
// Every other kind launches the head with the plain QuantGrid and carries neither the words nor the code.
struct QuantGridZ : QuantGrid {
    double* zpen;                             // [ntau][zrows]
    int zrow0, zrows;
    const double* sqd;                        // [ntau] sqrt(rows that carry a loss) of every fit (cross-validation folds), or NULL: sqrt(dim) for all
};
template <class GRID>
__device__ __forceinline__ void quant_fit_rows(DenseParams& q, const GRID& G, int fit) {
    if constexpr (std::is_same<GRID, QuantGridZ>::value) { if (G.sqd != nullptr) q.sqrt_dim = G.sqd[fit]; }
}
// slot s: every buffer of slot 0 shifted by s * stride doubles, its pair of control blocks behind slot 0's
__device__ __forceinline__ DenseParams quant_slot_params(DenseParams q, int s, long long stride) {
    const size_t o = (size_t)s * (size_t)stride;
    q.x += o; q.z0 += o; q.z1 += o; q.y0 += o; q.y1 += o; q.adj_z += o; q.adj_y += o; q.vec += o; q.P += o;
    q.Xz0 += o; q.Xz1 += o; q.Xy0 += o; q.Xy1 += o; q.u += o; q.cpart += o;
    q.ctl += 2 * s;
    return q;
}
// the control block of a cold start (pad: the slotted loop's index of the fit)
__host__ __device__ __forceinline__ DenseCtl dense_cold_ctl(double rho, int pad) {
    DenseCtl c;
    c.rho = rho; c.eps_primal = 0; c.eps_dual = 0; c.adj_a = 1.0; c.adj_c = 9999.0; c.tau = 0.0;
    c.restart = 0; c.iter = 0; c.done = 0; c.first = 1; c.total = 0; c.niter = 0; c.conv = 0; c.pad = pad;
    return c;
}
// One head launch for all slots: blockIdx.y = slot.  Every workgroup evaluates the decisions of ALL slots (as dense_head_kernel's
// workgroups all evaluate the one) and so knows, without atomics and the same on every run, which slots finish in this iteration and
// which quantile each of them takes next: the unclaimed ones are handed out in slot order.  A finishing slot records its quantile's
// niter, rho and get_x vector and starts the next quantile cold IN THIS LAUNCH (control block pad = the quantile's index): zero
// iterates, first = 1, rho = opts.rho.  With no quantile left it goes idle; when all are idle the sticky `done` word is set.
template <class GRID>
__global__ void __launch_bounds__(kDenseThreads)
quant_head_kernel(DenseParams q0, GRID G, int par) {
    __shared__ double sums[8];
    extern __shared__ __attribute__((aligned(16))) double pstage[];
    const int me = blockIdx.y;
    const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
    int next = load_flag_vector(G.next + par);
    DenseCtl in{};
    DenseDecision D{};
    int take = -1;
    bool all_idle = true;
    for (int s = 0; s < G.nslots; ++s) {
        DenseParams qs = quant_slot_params(q0, s, G.slot_stride);
        const DenseCtl cs = load_ctl_vector(qs.ctl + par);
        if (s == me) in = cs;
        if (cs.done) continue;                                   // idle (uniform)
        quant_fit_rows(qs, G, cs.pad);
        dense_head_sums(qs, pstage, sums);
        const DenseDecision Ds = dense_decide(qs, cs, sums);
        int tk = -1;
        if (Ds.out.done && next < G.ntau) tk = next++;
        if (!Ds.out.done || tk >= 0) all_idle = false;
        if (s == me) { D = Ds; take = tk; }
    }
    if (lead && me == 0) {
        G.next[par ^ 1] = next;
        if (all_idle) *q0.done = 1;
    }
    DenseParams q = quant_slot_params(q0, me, G.slot_stride);
    DenseCtl* outp = &q.ctl[par ^ 1];
    if (in.done) {
        if (lead) *outp = in;
        return;
    }
    const DenseCtl& out = D.out;
    if (!out.done) {
        if (lead) *outp = out;
        dense_head_vectors(q, in, out);
        return;
    }
    // the slot's quantile has finished.  Out of iterations: the last extrapolated pair, as the single run's head forms it
    if (D.write_adj) dense_head_vectors(q, in, out);
    const int k = in.pad;
    if (lead) { G.niter[k] = out.niter; G.rho_fin[k] = out.rho; }
    double* fin = G.fin + (size_t)k * G.fin_ld;
    if constexpr (std::is_same<GRID, QuantGridZ>::value) {
        // the latest z is the rows launch's of the finished iteration, in the slot the head calls `cur` (in.total is not advanced by a
        // finishing decision, converged or out of iterations): taken BEFORE the loop below zeroes it for the refill
        const double* zl = (in.total & 1) ? q.z1 : q.z0;
        double* zp = G.zpen + (size_t)k * G.zrows;
        for (int i = blockIdx.x * kDenseThreads + threadIdx.x; i < q.dim; i += gridDim.x * kDenseThreads)      // (the zeroing loop's mapping: a thread zeroes what it has read)
            if (i >= G.zrow0 && i - G.zrow0 < G.zrows) zp[i - G.zrow0] = zl[i];
    }
    for (int i = blockIdx.x * kDenseThreads + threadIdx.x; i < q.dim; i += gridDim.x * kDenseThreads) {      // (the mapping of dense_head_vectors: a thread reads what it wrote)
        fin[i] = q.data_vec[i] - q.adj_y[i] / out.rho + q.adj_z[i];                                          // lad_final_vec_kernel
        q.x[i] = 0; q.z0[i] = 0; q.z1[i] = 0; q.y0[i] = 0; q.y1[i] = 0;
    }
    if (take < 0) {
        if (lead) { *outp = out; G.idle[me] = 1; }
        return;
    }
    // the cold start of quantile `take`: what dense_init_kernel + the first head of a single run leave (the stale X'z, X'y of the other
    // parity and the stale partials are multiplied by zero or skipped under `first`, the norm partials are not read)
    const DenseCtl c0 = dense_cold_ctl(G.rho0, take);
    quant_fit_rows(q, G, take);
    const double zeros[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const DenseDecision D0 = dense_decide(q, c0, zeros);
    if (lead) *outp = D0.out;
    dense_head_vectors(q, c0, D0.out);
}

// LAD one-pass form: the rows of X (the stored transpose: row i is ld contiguous doubles) streamed ONCE.  A workgroup of eight waves
// owns a run of rows and takes them R at a time: every thread holds its 2 NPT columns of the R rows, the lanes' partial dots go through
// one halving butterfly per wave and the eight waves' sums through LDS (waves in order: a fixed order), every thread then knows
// x_i = row_i . s and forms z_i, y_i as the tail kernel does (same expressions, no contraction: the stepwise instrument replays them bit
// for bit), thread 0 stores them and adds up the six norms, and every thread adds row_i z_i, row_i y_i to its columns of X'z, X'y.
// The next R rows are requested before the current ones are reduced.
constexpr int kLadThreads = 512;
constexpr int kLadRows = 4;

// What lad_rows_kernel and quant_rows_kernel (S problems on one load of the rows) share: a problem in a slot is computed by exactly
// these functions, in the same order, as the same problem alone -- the two are bit-identical.
// the thread's 2 NPT entries of s = the g2 product's partial rows summed in order; the thread's X'z, X'y columns cleared
template <int NPT>
__device__ __forceinline__ void lad_load_s(const double* __restrict__ spart, int snseg, long long sstride, long long ld, int lp, int tid,
                                           double2 (&sv)[NPT], double2 (&az)[NPT], double2 (&ay)[NPT]) {
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
        const long long col = ((long long)k * kLadThreads + tid) * 2;
        double2 a = make_double2(0.0, 0.0);
        if (col < ld) for (int g = 0; g < snseg; ++g) { const double2 v = *reinterpret_cast<const double2*>(spart + (size_t)g * sstride + col); a.x += v.x; a.y += v.y; }
        if (col >= lp) a.x = 0.0;
        if (col + 1 >= lp) a.y = 0.0;
        sv[k] = a; az[k] = make_double2(0.0, 0.0); ay[k] = make_double2(0.0, 0.0);
    }
}
template <int R, int NPT>
__device__ __forceinline__ void lad_load_rows(const double* __restrict__ Xt, long long ld, int dim, int i0, int tid, double2 (&rv)[R][NPT]) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const double* row = Xt + (size_t)min(i0 + r, dim - 1) * ld;       // clamped: rows beyond the run are weighted with zero below
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
            const long long col = ((long long)k * kLadThreads + tid) * 2;
            rv[r][k] = col < ld ? load16_nt<double2>(row + col) : make_double2(0.0, 0.0);
        }
    }
}
// lane 8 r: the wave's sum of row_r . s
template <int R, int NPT>
__device__ __forceinline__ double lad_rows_dot(const double2 (&rv)[R][NPT], const double2 (&sv)[NPT], int lane) {
    double v8[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) v8[r] = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        double d = 0.0;
#pragma unroll
        for (int k = 0; k < NPT; ++k) { d = fma(rv[r][k].x, sv[k].x, d); d = fma(rv[r][k].y, sv[k].y, d); }
        v8[r] = d;
    }
    return halving_sum8(v8, lane);
}
// the entries of one problem's vectors a row needs (the same addresses in every lane)
struct LadRowIn { double ajy, ajz, zc; };
// row i with x_i = row_i . s known: z_i, y_i as the tail kernel forms them (same expressions, no contraction), thread 0 stores them and
// adds up the six norms, every thread adds row_i z_i, row_i y_i to its columns of X'z, X'y.  LANE_NORMS (the slotted kernel, to hold
// one accumulator per slot instead of six): thread k < 6 adds up norm k in nacc[0] -- the same squares added in the same order.
template <int NPT, bool LANE_NORMS, int PROX>
__device__ __forceinline__ void lad_row_step(int i, int tid, double x, double dv, const LadRowIn& in, double rho, double pen_hi, double pen_lo, double delta,
                                             double* __restrict__ xo, double* __restrict__ zn_, double* __restrict__ yn_,
                                             double* state, long long state_cap, int total, int dim,
                                             double* nacc, const double2 (&rv)[NPT], double2 (&az)[NPT], double2 (&ay)[NPT], double zlogit = 0.0, bool held = false) {
    double zn, yn;
    {
#pragma clang fp contract(off)
        if (kProxKinds[PROX].iterative) zn = zlogit;                         // formed once per row by the rows kernels' logit lanes, not in every thread
        else zn = prox2<PROX>(x - dv + in.ajy / rho, pen_hi, pen_lo, delta); // dense_tail_kernel, prob 0 (ADMMLAD.h:94-107)
        const double rr = x - dv - zn;
        yn = in.ajy + rho * rr;
        if (LANE_NORMS && tid < 6) {
            const double dz = zn - in.zc, daz = zn - in.ajz;
            const double t = tid == 0 ? rr : (tid == 1 ? dz : (tid == 2 ? daz : (tid == 3 ? x : (tid == 4 ? zn : yn))));
            if (!(kProxKinds[PROX].enet && held && tid >= 3)) nacc[0] += t * t;     // (held: a cross-validation fold's held-out row, row_held_out)
        }
        if (tid == 0) {
            if (!LANE_NORMS) {
                const double dz = zn - in.zc, daz = zn - in.ajz;
                nacc[0] += rr * rr; nacc[1] += dz * dz; nacc[2] += daz * daz;
                if (!(kProxKinds[PROX].enet && held)) { nacc[3] += x * x; nacc[4] += zn * zn; nacc[5] += yn * yn; }
            }
            xo[i] = x; zn_[i] = zn; yn_[i] = yn;
            if (state != nullptr && total < state_cap) {
                double* s = state + (size_t)total * 5 * dim;
                s[i] = x; s[(size_t)dim + i] = zn; s[2 * (size_t)dim + i] = yn; s[3 * (size_t)dim + i] = in.ajz; s[4 * (size_t)dim + i] = in.ajy;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
        az[k].x = fma(rv[k].x, zn, az[k].x); az[k].y = fma(rv[k].y, zn, az[k].y);
        ay[k].x = fma(rv[k].x, yn, ay[k].x); ay[k].y = fma(rv[k].y, yn, ay[k].y);
    }
}
// the workgroup's partial of X'z_new, X'y_new and its row of norm partials
template <int NPT, bool LANE_NORMS>
__device__ __forceinline__ void lad_store_partials(double* __restrict__ cpart, long long cstride, double* __restrict__ P, int tid,
                                                   const double2 (&az)[NPT], const double2 (&ay)[NPT], const double* nacc) {
    double* cz = cpart + ((size_t)blockIdx.x * 2) * cstride;
    double* cy = cz + cstride;
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
        const long long col = ((long long)k * kLadThreads + tid) * 2;
        if (col < cstride) { *reinterpret_cast<double2*>(cz + col) = az[k]; *reinterpret_cast<double2*>(cy + col) = ay[k]; }
    }
    double* Pout = P + (size_t)blockIdx.x * 8;
    if (LANE_NORMS) {
        if (tid < 6) Pout[tid] = nacc[0];
    } else if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) Pout[k] = nacc[k];
    }
}

template <int NPT, int PROX>
__global__ void __launch_bounds__(kLadThreads)
lad_rows_kernel(DenseParams q, int par, const double* __restrict__ Xt, long long ld, const double* __restrict__ spart, int snseg, long long sstride,
                double* __restrict__ cpart, int rows_per_wg, double knee) {
    constexpr int R = NPT <= 4 ? kLadRows : 2, NWV = kLadThreads / 64;      // (beyond 4096 columns two rows at a time: the registers hold two groups of rows)
    __shared__ double wsum[2][NWV][R];
    const DenseCtl c = load_ctl_vector(q.ctl + (par ^ 1));           // written by this iteration's head
    if (c.done) return;
    const int cur = (c.total - 1) & 1;
    const double* zc_ = cur ? q.z1 : q.z0;
    double* zn_ = cur ? q.z0 : q.z1; double* yn_ = cur ? q.y0 : q.y1;
    const double rho = c.rho, pen_hi = q.c_hi / rho, pen_lo = q.c_lo / rho;
    const double delta = PROX == kProxHuber ? knee : 0.0;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int row_lo = blockIdx.x * rows_per_wg, row_hi = min(q.dim, row_lo + rows_per_wg);
    double2 sv[NPT], az[NPT], ay[NPT];
    lad_load_s<NPT>(spart, snseg, sstride, ld, q.lp, tid, sv, az, ay);
    double nacc[6] = {0, 0, 0, 0, 0, 0};
    double2 ra[R][NPT], rb[R][NPT];
    int buf = 0;
    // kProxLogit.  The Newton prox is not formed in every thread (hundreds of double instructions a row against 8 NPT multiply-adds):
    // lane r of each wave forms row r's -- R proxes in the time of one -- and all lanes read it from there (two scalar reads, no
    // barrier).  To leave its registers free the four vectors' entries travel through LDS as in quant_rows_kernel: thread t < 4 R
    // requests ONE of them before the reduction.  x of a row is summed in the same order by the lane that forms the prox and by
    // lad_row_step's callers, and the prox's argument is lad_row_step's expression.  Rows beyond the run (clamped loads: finite) are
    // formed and dropped.
    // kProxLogitS: the response is identically zero there (x - 0 = x exactly, for every x), so the rows' label signs travel in its place.
    // kProxLogitR: the same, and a row whose sign is 0.0 (a ridge row: the last rows of the matrix) takes the square loss's prox instead.
    // kProxLogitE: the same with the elastic net's prox on those rows (q.c_hi, q.c_lo: the fit's constants; t of the +-1 rows stays 1 / rho).
    // kProxPoisE: the rows' counts travel there; a count >= 0 takes the Poisson prox, the marker -1.0 (a penalty row) the elastic net's.
    constexpr bool SIGNED = kProxKinds[PROX].tagged;
    __shared__ double uni[2][4 * R];           // d (kProxLogitS: the sign) | adj_y | adj_z | z of the R rows (unreferenced, so not allocated, in the other instantiations)
    auto group_logit = [&](int i0, const double2 (&rv)[R][NPT]) {
        double uval = 0.0;
        if (tid < 4 * R) {
            const int kind = tid / R, i = min(i0 + tid % R, q.dim - 1);
            const double* src = kind == 0 ? (SIGNED ? q.sgn : q.data_vec) : (kind == 1 ? q.adj_y : (kind == 2 ? q.adj_z : zc_));
            uval = src[i];
        }
        const double tot = lad_rows_dot<R, NPT>(rv, sv, lane);
        if ((lane & 7) == 0 && (lane >> 3) < R) wsum[buf][wid][lane >> 3] = tot;
        if (tid < 4 * R) uni[buf][tid] = uval;
        __syncthreads();
        double zl = 0.0;
        if (lane < R) {
#pragma clang fp contract(off)
            double x = wsum[buf][0][lane];
#pragma unroll
            for (int w = 1; w < NWV; ++w) x += wsum[buf][w][lane];
            if constexpr (SIGNED) zl = row_prox_tagged<PROX>(x + uni[buf][R + lane] / rho, [&] { return uni[buf][lane]; }, q.c_hi, q.c_lo, rho);
            else zl = prox2<PROX>(x - uni[buf][lane] + uni[buf][R + lane] / rho, pen_hi, pen_lo, delta);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = i0 + r;
            if (i >= row_hi) break;                                  // uniform
            double x = wsum[buf][0][r];
#pragma unroll
            for (int w = 1; w < NWV; ++w) x += wsum[buf][w][r];
            LadRowIn in;
            in.ajy = uni[buf][R + r]; in.ajz = uni[buf][2 * R + r]; in.zc = uni[buf][3 * R + r];
            lad_row_step<NPT, false, PROX>(i, tid, x, SIGNED ? 0.0 : uni[buf][r], in, rho, pen_hi, pen_lo, delta, q.x, zn_, yn_, q.state, q.state_cap, c.total, q.dim, nacc,
                                           rv[r], az, ay, read_lane_f64(zl, r), row_held_out<PROX>(uni[buf][r]));
        }
        buf ^= 1;
    };
    auto group = [&](int i0, const double2 (&rv)[R][NPT]) {
        if (kProxKinds[PROX].iterative) { group_logit(i0, rv); return; }
        // the four vectors' entries of the R rows (the same addresses in every lane), requested before the reduction
        double dv[R];
        LadRowIn in[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = min(i0 + r, q.dim - 1);
            dv[r] = q.data_vec[i]; in[r].ajy = q.adj_y[i]; in[r].ajz = q.adj_z[i]; in[r].zc = zc_[i];
        }
        const double tot = lad_rows_dot<R, NPT>(rv, sv, lane);      // lane 8 r: the wave's sum of row r
        if ((lane & 7) == 0 && (lane >> 3) < R) wsum[buf][wid][lane >> 3] = tot;
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = i0 + r;
            if (i >= row_hi) break;                                  // uniform
            double x = wsum[buf][0][r];
#pragma unroll
            for (int w = 1; w < NWV; ++w) x += wsum[buf][w][r];
            lad_row_step<NPT, false, PROX>(i, tid, x, dv[r], in[r], rho, pen_hi, pen_lo, delta, q.x, zn_, yn_, q.state, q.state_cap, c.total, q.dim, nacc, rv[r], az, ay);
        }
        buf ^= 1;                                                    // (the next group writes the other half of wsum: one barrier per group)
    };
    if (row_lo < row_hi) {
        lad_load_rows<R, NPT>(Xt, ld, q.dim, row_lo, tid, ra);
        for (int i0 = row_lo; i0 < row_hi; i0 += 2 * R) {
            if (i0 + R < row_hi) lad_load_rows<R, NPT>(Xt, ld, q.dim, i0 + R, tid, rb);
            group(i0, ra);
            if (i0 + R >= row_hi) break;
            if (i0 + 2 * R < row_hi) lad_load_rows<R, NPT>(Xt, ld, q.dim, i0 + 2 * R, tid, ra);
            group(i0 + R, rb);
        }
    }
    lad_store_partials<NPT, false>(cpart, q.cstride, q.P, tid, az, ay, nacc);
}

// S problems ("slots": the quantiles of admm_hip_quantreg's grid) on ONE load of every row group.  Slot s has its own s, prox constants,
// rho and control block, its own z / y / x / adj vectors, norm partials and X'z, X'y accumulators: all of slot 0's (q0) shifted by
// s * slot_stride doubles (control blocks: q0.ctl + 2 s).  A slot whose control block says done (idle: its last quantile has finished
// and none is left) does no work and stores nothing.
template <int NPT> struct QuantRowsR { static constexpr int value = NPT <= 2 ? kLadRows : 2; };
template <int NPT, int S, int PROX>
__global__ void __launch_bounds__(kLadThreads)
quant_rows_kernel(DenseParams q0, long long slot_stride, const double* __restrict__ chi, const double* __restrict__ clo, int par,
                  const double* __restrict__ Xt, long long ld, const double* __restrict__ spart0, int snseg, long long sstride,
                  double* __restrict__ cpart0, int rows_per_wg, const double* __restrict__ dlt) {
    constexpr int R = QuantRowsR<NPT>::value, NWV = kLadThreads / 64;
    // kProxLogitS (admm_hip_logit_multi: the slots are label columns): c_hi = c_lo = 1 and no knee, so chi / clo / dlt are not read; slot
    // s takes its rows' signs from column c.pad of the sign matrix q0.sgn (n x ncol, leading dimension n rounded up to 32) -- one more
    // per-slot entry of uni -- and the Newton prox is formed by lane s R + r of each wave for slot s, row r (see the group below).  The
    // shared response entry goes: the response is identically zero there and x - 0 = x exactly.
    // kProxLogitR (admm_hip_logit_ridge): the same; a prox lane whose row has sign 0.0 forms v (rho / (1 + rho)) with its slot's rho.
    // kProxLogitE (admm_hip_logit_enet: the slots are cells of a (column, lambda, alpha) grid, cell-major): chi / clo ARE read, by the fit
    // index c.pad, and the slot's label column is c.pad mod q0.sgn_cols; a prox lane whose row has sign 0.0 forms enet2 with its slot's
    // constants and rho.
    // kProxPoisE (admm_hip_poisson): kProxLogitE's indexing with the count matrix in the sign matrix's place; a prox lane whose row
    // carries a count >= 0 forms pois2 with its slot's rho, one whose row carries the marker -1.0 enet2.
    constexpr bool LOGIT = kProxKinds[PROX].tagged, ENET = kProxKinds[PROX].enet;
    constexpr int NV = LOGIT ? 4 : 3, NB = LOGIT ? 0 : 1;
    constexpr int NU = R * (NB + NV * S);                 // the vectors' entries a row group needs: d | per slot adj_y, adj_z, z   (LOGIT: no d; per slot also the sign)
    static_assert(!LOGIT || S * R <= 64, "one lane per slot and row");
    __shared__ double wsum[2][S][NWV][R];
    __shared__ double uni[2][NU];
    __shared__ double spen[2][S];                          // kProxLogitE: c_hi | c_lo of the fit the slot holds, for the prox lanes (written below, read behind a group's barrier; unreferenced, so not allocated, in the other instantiations)
    bool act[S];
    int cur[S];
    int col[S];                                            // (LOGIT) the slot's label column
    double rho[S], pen_hi[S], pen_lo[S], delta[S];         // (wave-uniform: the control block and the grid arrays are read as such)
    bool any = false;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const DenseCtl c = load_ctl_vector(q0.ctl + 2 * s + (par ^ 1));      // written by this iteration's head
        act[s] = !c.done; any = any || act[s];
        cur[s] = (c.total - 1) & 1;
        rho[s] = c.rho;
        const int k = act[s] ? c.pad : 0;                                    // the slot's place in the grid of quantiles
        if constexpr (ENET) {
            col[s] = k % q0.sgn_cols; pen_hi[s] = 0.0; pen_lo[s] = 0.0;
            if ((int)threadIdx.x == s) { spen[0][s] = chi[k]; spen[1][s] = clo[k]; }      // the fit's constants as they are (enet2 divides by its slot's rho), to LDS at once: no slot holds them in registers
        }
        else if constexpr (LOGIT) { col[s] = k; pen_hi[s] = 0.0; pen_lo[s] = 0.0; }
        else { pen_hi[s] = chi[k] / rho[s]; pen_lo[s] = clo[k] / rho[s]; }
        delta[s] = PROX == kProxHuber ? dlt[k] : 0.0;                        // the fit's knee travels with its c_hi / c_lo: by the index the head's refill hands over
    }
    if (!any) return;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int row_lo = blockIdx.x * rows_per_wg, row_hi = min(q0.dim, row_lo + rows_per_wg);
    // LOGIT: a prox lane needs the rho of ITS slot: through LDS (written here, read behind a group's barrier) and a mask of the live slots
    __shared__ double srho[S];
    unsigned live_slots = 0;
    if constexpr (LOGIT) {
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (tid == s) srho[s] = rho[s];
            live_slots |= act[s] ? 1u << s : 0u;
        }
    }
    double2 sv[S][NPT], az[S][NPT], ay[S][NPT];
    double nacc[S][1];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        nacc[s][0] = 0.0;
        if (act[s]) lad_load_s<NPT>(spart0 + s * slot_stride, snseg, sstride, ld, q0.lp, tid, sv[s], az[s], ay[s]);
    }
    double2 ra[R][NPT], rb[R][NPT];
    int buf = 0;
    auto group = [&](int i0, const double2 (&rv)[R][NPT]) {
        // the vectors' entries of the R rows: thread t < NU requests ONE of them before the reduction and passes it on through LDS
        // (held in every lane, as lad_rows_kernel holds its four per row, they would take the registers of a slot)
        double uval = 0.0;
        if (tid < NU) {
            const int kind = tid / R, i = min(i0 + tid % R, q0.dim - 1);
            const double* src = q0.data_vec;
            bool live = !LOGIT && kind == 0;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                if (kind == NB + NV * s) { src = q0.adj_y + (size_t)s * slot_stride; live = act[s]; }
                if (kind == NB + 1 + NV * s) { src = q0.adj_z + (size_t)s * slot_stride; live = act[s]; }
                if (kind == NB + 2 + NV * s) { src = (cur[s] ? q0.z1 : q0.z0) + (size_t)s * slot_stride; live = act[s]; }
                if constexpr (LOGIT) if (kind == NB + 3 + NV * s) { src = q0.sgn + (size_t)col[s] * (((size_t)q0.dim + 31) & ~(size_t)31); live = act[s]; }
            }
            if (live) uval = src[i];
        }
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (!act[s]) continue;
            const double tot = lad_rows_dot<R, NPT>(rv, sv[s], lane);
            if ((lane & 7) == 0 && (lane >> 3) < R) wsum[buf][s][wid][lane >> 3] = tot;
        }
        if (tid < NU) uni[buf][tid] = uval;
        __syncthreads();
        // LOGIT: lane s R + r of each wave forms the prox of slot s, row r -- the S R proxes of the group in the time of one -- and
        // every lane reads it from there, as lad_rows_kernel's logit group does for one slot.  The lane takes its slot's rho and its
        // entries of wsum / uni by address (a chain of selects over the per-slot registers became a table in LDS); x is summed in the order of the row loop
        // below.  An idle slot's lanes form nothing.
        double zl = 0.0;
        if constexpr (LOGIT) {
            const int ls = lane / R, lr = lane % R;
            if (lane < S * R && (live_slots >> ls & 1u)) {
#pragma clang fp contract(off)
                const double rho_l = srho[ls];
                double x = wsum[buf][ls][0][lr];
#pragma unroll
                for (int w = 1; w < NWV; ++w) x += wsum[buf][ls][w][lr];
                const double v = x + uni[buf][(NB + NV * ls) * R + lr] / rho_l;
                // the single fit's expressions with the slot's tag, constants and rho, as in lad_rows_kernel
                const auto tag = [&] { return uni[buf][(NB + 3 + NV * ls) * R + lr]; };
                if constexpr (ENET) zl = row_prox_tagged<PROX>(v, tag, spen[0][ls], spen[1][ls], rho_l);
                else zl = row_prox_tagged<PROX>(v, tag, 0.0, 0.0, rho_l);
            }
        }
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (!act[s]) continue;
            const size_t so = (size_t)s * slot_stride;
            double* zn_ = (cur[s] ? q0.z0 : q0.z1) + so; double* yn_ = (cur[s] ? q0.y0 : q0.y1) + so;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int i = i0 + r;
                if (i >= row_hi) break;                              // uniform
                double x = wsum[buf][s][0][r];
#pragma unroll
                for (int w = 1; w < NWV; ++w) x += wsum[buf][s][w][r];
                LadRowIn in;
                in.ajy = uni[buf][(NB + NV * s) * R + r]; in.ajz = uni[buf][(NB + 1 + NV * s) * R + r]; in.zc = uni[buf][(NB + 2 + NV * s) * R + r];
                double zrow = 0.0;
                bool held = false;
                if constexpr (LOGIT) zrow = read_lane_f64(zl, s * R + r);
                if constexpr (ENET) held = row_held_out<PROX>(uni[buf][(NB + 3 + NV * s) * R + r]);
                lad_row_step<NPT, true, PROX>(i, tid, x, LOGIT ? 0.0 : uni[buf][r], in, rho[s], pen_hi[s], pen_lo[s], delta[s], q0.x + so, zn_, yn_, nullptr, 0, 0, q0.dim, nacc[s], rv[r], az[s], ay[s], zrow, held);
            }
        }
        buf ^= 1;
    };
    if (row_lo < row_hi) {
        lad_load_rows<R, NPT>(Xt, ld, q0.dim, row_lo, tid, ra);
        for (int i0 = row_lo; i0 < row_hi; i0 += 2 * R) {
            if (i0 + R < row_hi) lad_load_rows<R, NPT>(Xt, ld, q0.dim, i0 + R, tid, rb);
            group(i0, ra);
            if (i0 + R >= row_hi) break;
            if (i0 + 2 * R < row_hi) lad_load_rows<R, NPT>(Xt, ld, q0.dim, i0 + 2 * R, tid, ra);
            group(i0 + R, rb);
        }
    }
#pragma unroll
    for (int s = 0; s < S; ++s)
        if (act[s]) lad_store_partials<NPT, true>(cpart0 + s * slot_stride, q0.cstride, q0.P + s * slot_stride, tid, az[s], ay[s], nacc[s]);
}

// BP one-pass form: B z_new for the z the tail of this iteration just wrote (gather over its non-zeros)
__global__ void __launch_bounds__(kGatherThreads)
bp_gather_kernel(DenseParams q, int par, GatherArgs<double> a) {
    const DenseCtl c = load_ctl_vector(q.ctl + (par ^ 1));
    if (c.done) return;
    const int cur = (c.total - 1) & 1;
    a.v = cur ? q.z0 : q.z1;                     // the tail wrote z_new into the buffer that is not `cur`
    gather_body<double>(a, (int)blockIdx.x, (int)blockIdx.y);
}

template <int PROX>
__global__ void __launch_bounds__(kDenseThreads)
dense_tail_kernel(DenseParams q, int par, double knee) {
    __shared__ double scratch[6 * (kDenseThreads / 64)];
    const DenseCtl c = load_ctl_vector(q.ctl + (par ^ 1));           // written by this iteration's head
    if (c.done) return;
    const int cur = (c.total - 1) & 1;           // head already advanced `total`
    const double* zc_ = cur ? q.z1 : q.z0;
    double* zn_ = cur ? q.z0 : q.z1; double* yn_ = cur ? q.y0 : q.y1;
    const double rho = c.rho, pen_hi = q.c_hi / rho, pen_lo = q.c_lo / rho;
    const double delta = PROX == kProxHuber ? knee : 0.0;
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (int i = blockIdx.x * kDenseThreads + threadIdx.x; i < q.dim; i += gridDim.x * kDenseThreads) {
#pragma clang fp contract(off)
        double g = 0.0;
        for (int s = 0; s < q.gout_nseg; ++s) g += q.gout[(size_t)s * q.gout_stride + i];
        const double adjy = q.adj_y[i], adjz = q.adj_z[i], zc = zc_[i];
        double x, zn, r;
        bool held = false;
        if (q.prob == 0) {                        // LAD: x = P_X(vec); z = prox(x - y + adj_y/rho; c_hi/rho, c_lo/rho); r = x - y - z
            x = g;
            const double d = q.data_vec[i];
            if constexpr (kProxKinds[PROX].tagged) {
                const double tg = q.sgn[i];
                held = row_held_out<PROX>(tg);
                zn = row_prox_tagged<PROX>(x - d + adjy / rho, [tg] { return tg; }, q.c_hi, q.c_lo, rho);
            } else zn = prox2<PROX>(x - d + adjy / rho, pen_hi, pen_lo, delta);
            r = x - d - zn;
        } else {                                  // BP: x = vec + A'(AA')^-1 b - B'(B vec); z = soft(x + adj_y/rho, 1/rho); r = x - z
            x = q.vec[i] + q.data_vec[i] - g;
            zn = soft2(x + adjy / rho, pen_hi, pen_lo);
            r = x - zn;
        }
        const double yn = adjy + rho * r;
        const double dz = zn - zc, daz = zn - adjz;
        acc[0] += r * r; acc[1] += dz * dz; acc[2] += daz * daz;
        if (!held) { acc[3] += x * x; acc[4] += zn * zn; acc[5] += yn * yn; }
        q.x[i] = x; zn_[i] = zn; yn_[i] = yn;
        if (q.state != nullptr && c.total < q.state_cap) {     // record c.total = the trace record that will judge this iteration
            double* s = q.state + (size_t)c.total * 5 * q.dim;
            s[i] = x; s[(size_t)q.dim + i] = zn; s[2 * (size_t)q.dim + i] = yn; s[3 * (size_t)q.dim + i] = adjz; s[4 * (size_t)q.dim + i] = adjy;
        }
    }
    block_sum<double, 6>(acc, scratch);
    if (threadIdx.x == 0) {
        double* Pout = q.P + (size_t)blockIdx.x * 8;
#pragma unroll
        for (int k = 0; k < 6; ++k) Pout[k] = acc[k];
    }
}

__global__ void dense_init_kernel(DenseParams q, double rho) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < q.dim) { q.x[i] = 0; q.z0[i] = 0; q.z1[i] = 0; q.y0[i] = 0; q.y1[i] = 0; q.adj_z[i] = 0; q.adj_y[i] = 0; q.vec[i] = 0; }
    if (i < q.nwg_tail * 8) q.P[i] = 0.0;
    if (i == 0) {
        const DenseCtl c = dense_cold_ctl(rho, 0);
        q.ctl[0] = c; q.ctl[1] = c;
        *q.done = 0;
    }
}

// vec = y - adj_y / rho + adj_z for LAD's get_x (ADMMLAD.h:220-225)
__global__ void lad_final_vec_kernel(const double* y, const double* adj_y, const double* adj_z, double rho, int n, double* vec) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) vec[i] = y[i] - adj_y[i] / rho + adj_z[i];
}

__global__ void __launch_bounds__(1024)
norm2_kernel(const double* v, int n, double* out) {
    __shared__ double scratch[16];
    double s[1] = {0.0};
    for (int i = threadIdx.x; i < n; i += 1024) s[0] += v[i] * v[i];
    block_sum<double, 1>(s, scratch);
    if (threadIdx.x == 0) out[0] = sqrt(s[0]);
}

namespace {

// Kernel selection: f(std::integral_constant<int, V>) for the V of the compile-time range LO .. HI that equals the runtime v; false
// if there is none (an empty range included).  Nested over kind, NPT and S with the bounds read from kProxKinds, this instantiates
// exactly the kernels the table admits.
template <int LO, int HI, class F>
bool with_constant(int v, const F& f) {
    if constexpr (LO > HI) return false;
    else {
        if (v != LO) return with_constant<LO + 1, HI>(v, f);
        f(std::integral_constant<int, LO>{});
        return true;
    }
}

struct DenseLoop {
    DevBuf<double> x, z0, z1, y0, y1, adj_z, adj_y, vec, P;
    DevBuf<DenseCtl> ctl;
    DevBuf<int> done;
    DenseParams q{};
    int nwg_head = 0;
    int prox = kProxSoft;                      // the tail's prox (prob 0; BP keeps the soft-threshold)
    double delta = 0.0;                        // its knee (kProxHuber)
    DevBuf<double> trace, state;

    void init(int dim, int prob, const admm_opts& o, const double* data_vec, double extra_norm, hipStream_t st, long long trace_cap = 0, long long state_cap = 0,
              int norm_rows = 0) {      // norm_rows > 0: that many rows of norm partials (the launch that forms them is not dense_tail_kernel)
        const long long ld = round_up(dim, 32);
        for (DevBuf<double>* b : {&x, &z0, &z1, &y0, &y1, &adj_z, &adj_y, &vec}) { b->alloc(ld); b->zero(st); }
        const int nwg_tail = norm_rows > 0 ? norm_rows : std::max(1, std::min(64, (dim + kDenseThreads - 1) / kDenseThreads));
        nwg_head = std::max(1, std::min(device_info().num_cu, (dim + kDenseThreads - 1) / kDenseThreads));
        P.alloc((size_t)nwg_tail * 8); ctl.alloc(2); done.alloc(1);
        q.dim = dim; q.prob = prob; q.maxit = o.maxit; q.nwg_tail = nwg_tail;
        q.eps_abs = o.eps_abs; q.eps_rel = o.eps_rel; q.sqrt_dim = std::sqrt((double)dim); q.extra_norm = extra_norm;
        q.data_vec = data_vec;
        q.c_hi = 1.0; q.c_lo = 1.0;
        q.x = x.get(); q.z0 = z0.get(); q.z1 = z1.get(); q.y0 = y0.get(); q.y1 = y1.get();
        q.adj_z = adj_z.get(); q.adj_y = adj_y.get(); q.vec = vec.get();
        q.ctl = ctl.get(); q.P = P.get(); q.done = done.get();
        if (trace_cap > 0) { trace.alloc((size_t)trace_cap * ADMM_TRACE_FIELDS); q.trace = trace.get(); q.trace_cap = trace_cap; }
        if (state_cap > 0) {     // iterate dump; record 0 (the cold start has no iterates) carries data_vec as this solver holds it, in the x slot
            state.alloc((size_t)state_cap * 5 * dim);
            ADMM_HIP_CHECK(hipMemsetAsync(state.get(), 0, (size_t)state_cap * 5 * dim * sizeof(double), st));
            ADMM_HIP_CHECK(hipMemcpyAsync(state.get(), data_vec, (size_t)dim * sizeof(double), hipMemcpyDeviceToDevice, st));
            q.state = state.get(); q.state_cap = state_cap;
        }
        const int init_n = std::max(dim, nwg_tail * 8);
        hipLaunchKernelGGL(dense_init_kernel, dim3((init_n + 255) / 256), dim3(256), 0, st, q, o.rho);
    }
    void head(long long g, hipStream_t st) {
        hipLaunchKernelGGL(dense_head_kernel, dim3(nwg_head), dim3(kDenseThreads), (size_t)q.nwg_tail * 8 * sizeof(double), st, q, (int)(g & 1));
    }
    void tail(long long g, hipStream_t st) {
        const bool found = with_constant<0, kProxKindCount - 1>(prox, [&](auto kind) {      // (the knee is read by the Huber instantiation alone)
            hipLaunchKernelGGL(dense_tail_kernel<decltype(kind)::value>, dim3(q.nwg_tail), dim3(kDenseThreads), 0, st, q, (int)(g & 1), delta);
        });
        if (!found) throw Error(ADMM_ERR_INTERNAL, "dense loop: no tail kernel for this prox");
    }
    DenseCtl final_ctl(hipStream_t st) {
        DenseCtl h[2];
        ADMM_HIP_CHECK(hipMemcpyAsync(h, ctl.get(), sizeof(h), hipMemcpyDeviceToHost, st));
        ADMM_HIP_CHECK(hipStreamSynchronize(st));
        return h[0].done ? h[0] : h[1];
    }
};


}  // namespace

__global__ void __launch_bounds__(256) copy_cols_f64_kernel(const double* __restrict__ in, long long ldi, int rows, double* __restrict__ out, long long ldo) {
    const int c = blockIdx.y;
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r < rows) out[(size_t)c * ldo + r] = in[(size_t)c * ldi + r];
}

// ---------------------------------------------------------------------------------------------- LAD
// copies the decision records of a finished loop into the result
static void dense_collect_trace(DenseLoop& L, const DenseCtl& fc, DenseResult& res, hipStream_t st) {
    if (res.trace_cap <= 0) return;
    const long long taken = fc.total + (fc.done ? 1 : 0);      // the finishing decision does not advance `total`
    collect_records(res.trace, L.trace.get(), ADMM_TRACE_FIELDS, taken, res.trace_cap, st);
    if (res.state_cap > 0) {                                   // one record per decision, same numbering as the trace
        res.state_dim = L.q.dim;
        collect_records(res.state, L.state.get(), 5ll * L.q.dim, taken, res.state_cap, st);
    }
}

namespace {

// columns a thread of the rows kernels holds per row (kProxKinds' max_slots is indexed by it)
inline int lad_npt(long long ldxt) { return (int)((ldxt / 2 + kLadThreads - 1) / kLadThreads); }

// The separable loss of one fit, as the loop sees it: which prox, its weights above / below zero, and (Huber) the knee in the units
// of the standardised response.  LAD: the default.
struct LadProx {
    int kind = kProxSoft;
    double c_hi = 1.0, c_lo = 1.0, delta = 0.0;
    const double* signs = nullptr;             // kProxLogit: the n label signs folded into the matrix (device), for the iterate dump
                                               // kProxLogitS: the signs the prox reads -- fit k's is column k of ONE matrix, leading dimension round_up(n, 32)
                                               // kProxLogitR: the same over the augmented rows, 0.0 on the ridge rows
                                               // kProxLogitE: the same; fit k's column is k mod ncols of the matrix at fits[0].signs, and c_hi / c_lo are the penalty rows' constants
                                               // kProxPoisE: the E form's layout with the counts in the signs' place, -1.0 on the penalty rows and the padding
    int ncols = 0;                             // kProxLogitE, kProxPoisE: the label (count) columns of the sign matrix
    int live_rows = 0;                         // cross-validation folds: the rows that carry a loss (all but the held-out ones), the `rows` of the stop thresholds; 0: all
};

// M = G0 + lambda D, D = 1 on the first p0 diagonal entries (the user's columns; the intercept's entry is not shifted): one pass, both
// ld x ld, padding included
__global__ void __launch_bounds__(256) ridge_gram_kernel(const double* __restrict__ G0, double* __restrict__ M, long long ld, int p0, double lambda) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= ld * ld) return;
    const long long r = i % ld, c = i / ld;
    const double g = G0[i];
    M[i] = r == c && r < p0 ? g + lambda : g;
}
// the p0 non-zeros of the ridge rows sqrt(lambda) e_j' (rows n0 + j, j < p0) in the column-major X and in its stored transpose
__global__ void __launch_bounds__(256) ridge_rows_kernel(double* __restrict__ X, long long ldx, double* __restrict__ Xt, long long ldxt, int n0, int p0, double root) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= p0) return;
    X[(size_t)j * ldx + n0 + j] = root;
    Xt[((size_t)n0 + j) * ldxt + j] = root;
}

// Everything of a LAD-type fit that does not depend on the prox constants, formed ONCE (setup), and the loop from a cold start
// (loop: one quantile; loop_slots: a grid, several quantiles per pass over X).  admm_hip_lad is setup + one loop with c_hi = c_lo = 1.
struct LadProblem {
    const DeviceData<double>& d;
    const admm_opts& opts;
    hipStream_t st;
    int n, p;
    long long ldp, ldxt, ldh = 0;
    bool hat = false, onepass = false;
    int lad_nwg = 1, lad_rows = 0;
    double ynorm = 0;
    DevBuf<double> M, Xt, H, Xd, tvec, svec;
    GemvT<double> g1, g2, g3, gH;                // t = X' vec ; s = (X'X)^-1 t ; xs = X s ;  or xs = H vec
    int n0 = 0, ridge_p0 = 0;                    // ridge rows (setup_ridge): the data rows and the ridge rows behind them, n = n0 + ridge_p0
    DevBuf<double> G0;                           // ... and the Gram matrix of the data rows

    LadProblem(const DeviceData<double>& d_, const admm_opts& o, hipStream_t st_) : d(d_), opts(o), st(st_), n(d_.n), p(d_.p) {}

    // setup = the Gram matrix | its inverse | the stored transpose | everything behind them (finish_setup).  A lambda grid of ridge rows
    // (setup_ridge / setup_lambda below) pays the first and the third once and the other two per lambda.
    // the Gram matrix of the first `rows` rows of X into G (ldp x ldp)
    void form_gram(DevBuf<double>& G, int rows, admm_stats& S) {
        ldp = round_up(p, 128);                // whole 128-blocks for the matrix-core inverse
        const double t0 = now_s();
        G.alloc((size_t)ldp * ldp); G.zero(st);
        gram_full<double>(d.X.get(), d.ldx, rows, p, true, G.get(), ldp, st);
        ADMM_HIP_CHECK(hipStreamSynchronize(st));
        S.t_gram = now_s() - t0;
    }
    // M -> its inverse; n <= 2000: the hat-matrix branch also needs the Cholesky factor of the same Gram matrix: G2 keeps a copy
    void invert_gram(DevBuf<double>& G2) {
        hat = n <= 2000;
        if (opt_off(Opt::LAD_HAT)) hat = false;
        if (hat) {
            G2.alloc((size_t)ldp * ldp);
            ADMM_HIP_CHECK(hipMemcpyAsync(G2.get(), M.get(), (size_t)ldp * ldp * sizeof(double), hipMemcpyDeviceToDevice, st));
        }
        spd_inverse_f64(M.get(), ldp, p, st);
    }
    void form_transpose() {
        ldxt = round_up(p, 32);
        Xt.alloc((size_t)ldxt * n); Xt.zero(st);
        transpose<double>(d.X.get(), d.ldx, n, p, Xt.get(), ldxt, st);
    }

    void setup(admm_stats& S) {
        // X'X, its inverse (LLT of X'X in the reference, ADMMLAD.h:186-189), X' stored for the X*s product
        form_gram(M, n, S);
        const double t0 = now_s();
        DevBuf<double> G2;
        invert_gram(G2);
        form_transpose();
        ADMM_HIP_CHECK(hipStreamSynchronize(st));
        S.t_factor = now_s() - t0;
        finish_setup(S, G2);
    }

    // Ridge rows (solve_logit_ridge): d.X holds n0 data rows and, behind them, p0 rows that are zero until setup_lambda writes
    // sqrt(lambda) e_j' into them.  Once per call: G0 = the Gram matrix of the DATA rows, and the transpose.
    void setup_ridge(int n0_, int p0_, admm_stats& S) {
        n0 = n0_; ridge_p0 = p0_;
        form_gram(G0, n0, S);
        const double t0 = now_s();
        M.alloc((size_t)ldp * ldp);
        form_transpose();
        ADMM_HIP_CHECK(hipStreamSynchronize(st));
        S.t_factor = now_s() - t0;
    }
    // Per lambda: M = G0 + lambda D (the Gram matrix of the augmented rows, D = 1 on the p0 user columns), the p0 entries of the ridge
    // rows in X and in its transpose, and what setup does behind the Gram matrix.
    void setup_lambda(double lambda, admm_stats& S) {
        const double t0 = now_s();
        hipLaunchKernelGGL(ridge_gram_kernel, dim3((unsigned)(((size_t)ldp * ldp + 255) / 256)), dim3(256), 0, st, G0.get(), M.get(), ldp, ridge_p0, lambda);
        hipLaunchKernelGGL(ridge_rows_kernel, dim3((ridge_p0 + 255) / 256), dim3(256), 0, st, d.X.get(), d.ldx, Xt.get(), ldxt, n0, ridge_p0, std::sqrt(lambda));
        DevBuf<double> G2;
        invert_gram(G2);
        ADMM_HIP_CHECK(hipStreamSynchronize(st));
        S.t_factor += now_s() - t0;
        finish_setup(S, G2);
    }

    void finish_setup(admm_stats& S, DevBuf<double>& G2) {
        double t0;
        DevBuf<double> ynorm_d(1);
        hipLaunchKernelGGL(norm2_kernel, dim3(1), dim3(1024), 0, st, d.Y.get(), n, ynorm_d.get());
        ADMM_HIP_CHECK(hipMemcpyAsync(&ynorm, ynorm_d.get(), sizeof(double), hipMemcpyDeviceToHost, st));
        ADMM_HIP_CHECK(hipStreamSynchronize(st));

        // general branch, one-pass form (DenseParams::lp): X streamed once per iteration by rows.  LAD_ONEPASS=0: the reference's two products.
        constexpr int kLadMaxCols = 2 * kLadThreads * kLadMaxNpt;            // 6144 columns: six double2 per thread and row (more would spill)
        onepass = !hat && p <= kLadMaxCols;
        if (opt_off(Opt::LAD_ONEPASS)) onepass = false;
        lad_nwg = std::max(1, std::min(device_info().num_cu, (n + 2 * kLadRows - 1) / (2 * kLadRows)));
        lad_rows = (int)round_up((n + lad_nwg - 1) / lad_nwg, kLadRows);

        g1.init(d.X.get(), d.ldx, n, p);
        g2.init(M.get(), ldp, p, p);
        tvec.alloc(ldp); svec.alloc(ldp);
        tvec.zero(st); svec.zero(st);

        // n <= 2000: the reference caches the hat matrix H = X (X'X)^-1 X' = T T', T = X L^-T, and projects with one
        // symmetric product (ADMMLAD.h:67-73,191-203).  Same here: T = X U with U = L^-T from the blocked factorisation,
        // H = T T' on the fp64 matrix cores, then ONE mat-vec per iteration.  ADMM_HIP_LAD_HAT=0 keeps the general form.
        if (hat) {
            t0 = now_s();
            const long long ldn = round_up(n, 128);
            const int pk = (int)round_up(p, 8);
            DevBuf<double> U = cholesky_linvt_mfma_f64(G2.get(), ldp, p, st);          // U = L^-T (p x p, upper)
            DevBuf<double> W((size_t)ldp * ldp), Xp((size_t)ldn * pk), T((size_t)ldn * ldp);
            Xp.zero(st); T.zero(st);
            transpose<double>(U.get(), ldp, (int)ldp, (int)ldp, W.get(), ldp, st);      // W = L^-1: W[j, k] = U[k, j]
            hipLaunchKernelGGL(copy_cols_f64_kernel, dim3((n + 255) / 256, p), dim3(256), 0, st, d.X.get(), d.ldx, n, Xp.get(), ldn);
            gemm_nt_f64(Xp.get(), ldn, W.get(), ldp, T.get(), ldn, n, p, pk, st, true); // T[i, j] = sum_k X[i, k] U[k, j]   (W = U' = L^-1: lower triangular)
            ldh = ldn;
            H.alloc((size_t)ldh * ldh); H.zero(st);
            gram_full<double>(T.get(), ldn, n, p, false, H.get(), ldh, st);             // H = T T' (tcross_prod_lower)
            ADMM_HIP_CHECK(hipStreamSynchronize(st));
            S.t_factor += now_s() - t0;
            gH.init(H.get(), ldh, n, n);
            gH.set_nt(gemv_stream_nt(gH.bytes()));
        } else if (!onepass) {
            g3.init(Xt.get(), ldxt, p, n);
            const bool nt = gemv_stream_nt(g1.bytes() + g2.bytes() + g3.bytes());        // per iteration: X', the inverse, X
            g1.set_nt(nt); g2.set_nt(nt); g3.set_nt(nt);
        }
        if (onepass) {
            g2.set_nt(gemv_stream_nt(g1.bytes() + g2.bytes()));
            Xd.alloc(ldp); Xd.zero(st);
            g1.run(d.Y.get(), Xd.get(), nullptr, st);                // X'd, once
        }
    }

    // get_x(): (X'X)^-1 X' vec for vec = y - adj_y/rho + adj_z with the final adj and rho (ADMMLAD.h:220-225), on the host
    void coef_of(const double* vec, double* coef) {
        g1.run(vec, tvec.get(), nullptr, st);
        g2.run(tvec.get(), svec.get(), nullptr, st);
        ADMM_HIP_CHECK(hipMemcpyAsync(coef, svec.get(), (size_t)p * sizeof(double), hipMemcpyDeviceToHost, st));
        ADMM_HIP_CHECK(hipStreamSynchronize(st));
    }

    // One loop from a cold start with the prox px; coef: the p coefficients of the standardised problem.  Returns niter.
    // zpen (kProxLogitE): the ridge_p0 penalty-row entries of the last z, the prox output of the final iteration.
    int loop(const LadProx& px, DenseResult& res, double* coef, double* zpen = nullptr) {
        admm_stats& S = res.stats;
        DenseLoop L;
        L.init(n, 0, opts, d.Y.get(), ynorm, st, res.trace_cap, res.state_cap, onepass ? lad_nwg : 0);
        L.q.c_hi = px.c_hi; L.q.c_lo = px.c_lo; L.delta = px.delta; L.prox = px.kind;
        if (px.live_rows > 0) L.q.sqrt_dim = std::sqrt((double)px.live_rows);
        if (kProxKinds[px.kind].tagged) L.q.sgn = px.signs;
        if (px.kind == kProxHuber && res.state_cap > 0) {       // iterate dump: record 0 also carries the knee as the loop holds it (delta / scaleY), first entry of its z slot
            ADMM_HIP_CHECK(hipMemcpyAsync(L.state.get() + n, &px.delta, sizeof(double), hipMemcpyHostToDevice, st));
            ADMM_HIP_CHECK(hipStreamSynchronize(st));
        }
        if ((px.kind == kProxLogit || px.kind == kProxLogitR || kProxKinds[px.kind].enet) && res.state_cap > 0)      // the same for the logistic fit: the n signs the loop ran with fill record 0's z slot (ridge rows: 0.0; kProxPoisE: the counts, penalty rows -1.0)
            ADMM_HIP_CHECK(hipMemcpyAsync(L.state.get() + n, px.signs, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
        if (hat) { L.q.gout = gH.part.get(); L.q.gout_nseg = gH.pl.nseg; L.q.gout_stride = gH.stride; }
        else if (!onepass) { L.q.gout = g3.part.get(); L.q.gout_nseg = g3.pl.nseg; L.q.gout_stride = g3.stride; }
        DevBuf<double> Xz0, Xz1, Xy0, Xy1, uvec, cpart;
        if (onepass) {
            for (DevBuf<double>* b : {&Xz0, &Xz1, &Xy0, &Xy1, &uvec}) { b->alloc(ldp); b->zero(st); }
            cpart.alloc((size_t)lad_nwg * 2 * ldp); cpart.zero(st);
            L.q.lp = p; L.q.Xd = Xd.get(); L.q.Xz0 = Xz0.get(); L.q.Xz1 = Xz1.get(); L.q.Xy0 = Xy0.get(); L.q.Xy1 = Xy1.get(); L.q.u = uvec.get();
            L.q.cpart = cpart.get(); L.q.cnwg = lad_nwg; L.q.cstride = ldp;
        }
        auto launch_rows = [&](long long g) {
            const int par = (int)(g & 1);
            bool found = false;
            with_constant<0, kProxKindCount - 1>(px.kind, [&](auto kind) {
                found = with_constant<1, kLadMaxNpt>(std::min(lad_npt(ldxt), kLadMaxNpt), [&](auto npt) {
                    hipLaunchKernelGGL((lad_rows_kernel<decltype(npt)::value, decltype(kind)::value>), dim3(lad_nwg), dim3(kLadThreads), 0, st, L.q, par, Xt.get(), ldxt,
                                       g2.part.get(), g2.pl.nseg, g2.stride, cpart.get(), lad_rows, px.delta);
                });
            });
            if (!found) throw Error(ADMM_ERR_INTERNAL, "one-pass loop: no rows kernel for this prox");
        };

        const int* skip = L.done.get();
        LoopTimes lt = run_until_done(st, skip, batch_iters((int)opt_int(Opt::BATCH_ITERS, 0), 8), (long long)opts.maxit + 2, [&](long long g) {
            L.head(g, st);
            if (hat) {
                gH.run_partials(L.vec.get(), skip, st);          // dsymv(H, vec)
            } else if (onepass) {
                g2.run_partials(uvec.get(), skip, st);           // s = (X'X)^-1 u, u = X'vec formed by the head from X'd, X'z, X'y
                launch_rows(g);                                   // x = X s, z, y, norms, X'z_new, X'y_new: one pass over the rows of X
                return;
            } else {
                g1.run_partials(L.vec.get(), skip, st);          // chained: the next product sums these partial rows while staging
                g2.run_partials_from(g1, skip, st);
                g3.run_partials_from(g2, skip, st);
            }
            L.tail(g, st);
        });
        S.t_loop += lt.wall_s; S.loop_ms_events += lt.events_ms; S.xupdate_launches += lt.launched;

        const DenseCtl fc = L.final_ctl(st);
        S.total_iter += fc.niter; S.rho = fc.rho;
        S.xupdate_variant = onepass ? 1 : 0;
        dense_collect_trace(L, fc, res, st);
        hipLaunchKernelGGL(lad_final_vec_kernel, dim3((n + 255) / 256), dim3(256), 0, st, d.Y.get(), L.adj_y.get(), L.adj_z.get(), fc.rho, n, L.vec.get());
        coef_of(L.vec.get(), coef);
        if (zpen != nullptr)     // get_z() of the finished loop (solve_bp reads it the same way), the penalty rows' part
            read_back(zpen, ((fc.total & 1) ? L.z1.get() : L.z0.get()) + n0, (size_t)ridge_p0 * sizeof(double), st);
        return fc.niter;
    }

    // A grid of quantiles, S >= 2 of them per pass over X (one-pass branch only).  Per iteration: quant_head_kernel for all slots, ONE
    // batched launch of the slots' (X'X)^-1 u products (g2's plan: the partials of the single run), quant_rows_kernel.  The slots refill
    // on the device; the host polls the one `done` word.  fits: the grid, all of one prox kind.  coef: [ntau][p].
    void loop_slots(int S_, const std::vector<LadProx>& fits, admm_stats& S, int* niter, double* coef, double* zpen = nullptr) {
        const int ntau = (int)fits.size(), nslots = S_;
        const int kind = fits[0].kind;
        std::vector<double> c_hi(ntau), c_lo(ntau), dlt(ntau);
        for (int k = 0; k < ntau; ++k) { c_hi[k] = fits[k].c_hi; c_lo[k] = fits[k].c_lo; dlt[k] = fits[k].delta; }
        const long long ldn = round_up(n, 32);
        const size_t gpart_sz = (size_t)g2.pl.nseg * g2.stride;
        // one slot: 8 n-vectors | X'z (2), X'y (2), u | norm partials | the rows launch's partials | the product's partial rows
        const size_t o_p = 8 * (size_t)ldn, o_P = o_p + 5 * (size_t)ldp, o_c = o_P + (size_t)lad_nwg * 8, o_g = o_c + (size_t)lad_nwg * 2 * ldp;
        const size_t stride = round_up_sz(o_g + gpart_sz, 32);
        DevBuf<double> pool(stride * nslots), fin((size_t)ntau * ldn), chi_d(ntau), clo_d(ntau), dlt_d(ntau), rho_fin(ntau);
        DevBuf<DenseCtl> ctl(2 * (size_t)nslots);
        DevBuf<int> ints(3 + nslots + ntau);                     // done | next[2] | idle[nslots] | niter[ntau]
        DevBuf<GemvTArgs<double>> batch(nslots);
        pool.zero(st); fin.zero(st); rho_fin.zero(st);
        std::vector<int> hi(3 + nslots + ntau, 0);
        hi[1] = hi[2] = nslots;                                  // slots 0 .. S-1 start with the first S quantiles
        std::vector<DenseCtl> hc(2 * (size_t)nslots);
        for (int s = 0; s < nslots; ++s) hc[2 * s] = hc[2 * s + 1] = dense_cold_ctl(opts.rho, s);
        DenseParams q{};
        double* b = pool.get();
        q.dim = n; q.prob = 0; q.maxit = opts.maxit; q.nwg_tail = lad_nwg;
        q.eps_abs = opts.eps_abs; q.eps_rel = opts.eps_rel; q.sqrt_dim = std::sqrt((double)n); q.extra_norm = ynorm;
        q.data_vec = d.Y.get();
        q.x = b; q.z0 = b + ldn; q.z1 = b + 2 * ldn; q.y0 = b + 3 * ldn; q.y1 = b + 4 * ldn; q.adj_z = b + 5 * ldn; q.adj_y = b + 6 * ldn; q.vec = b + 7 * ldn;
        q.ctl = ctl.get(); q.P = b + o_P; q.done = ints.get();
        q.lp = p; q.Xd = Xd.get(); q.Xz0 = b + o_p; q.Xz1 = b + o_p + ldp; q.Xy0 = b + o_p + 2 * ldp; q.Xy1 = b + o_p + 3 * ldp; q.u = b + o_p + 4 * ldp;
        q.cpart = b + o_c; q.cnwg = lad_nwg; q.cstride = ldp;
        q.c_hi = 1.0; q.c_lo = 1.0;                              // (unused: the slots' constants are chi / clo of their quantile)
        if (kProxKinds[kind].tagged) q.sgn = fits[0].signs;         // the sign matrix: a slot reads the column of the fit it holds
        q.sgn_cols = kProxKinds[kind].enet ? fits[0].ncols : 0;
        DevBuf<double> zpen_d, sqd_d;
        QuantGridZ G{};
        if (kProxKinds[kind].enet) {
            zpen_d.alloc((size_t)ntau * ridge_p0); zpen_d.zero(st);
            G.zpen = zpen_d.get(); G.zrow0 = n0; G.zrows = ridge_p0;
            if (fits[0].live_rows > 0) {
                std::vector<double> hs(ntau);
                for (int k = 0; k < ntau; ++k) hs[k] = std::sqrt((double)fits[k].live_rows);
                sqd_d.alloc(ntau);
                write_device(sqd_d.get(), hs.data(), (size_t)ntau * sizeof(double));
                G.sqd = sqd_d.get();
            }
        }
        G.nslots = nslots; G.ntau = ntau; G.slot_stride = (long long)stride; G.rho0 = opts.rho;
        G.next = ints.get() + 1; G.idle = ints.get() + 3; G.niter = ints.get() + 3 + nslots; G.rho_fin = rho_fin.get();
        G.fin = fin.get(); G.fin_ld = ldn;
        std::vector<GemvTArgs<double>> hb(nslots);
        for (int s = 0; s < nslots; ++s) {
            hb[s] = g2.args_partials(q.u + s * stride, G.idle + s);
            hb[s].out[0] = b + s * stride + o_g;
        }
        ADMM_HIP_CHECK(hipMemcpyAsync(ints.get(), hi.data(), hi.size() * sizeof(int), hipMemcpyHostToDevice, st));
        ADMM_HIP_CHECK(hipMemcpyAsync(ctl.get(), hc.data(), hc.size() * sizeof(DenseCtl), hipMemcpyHostToDevice, st));
        ADMM_HIP_CHECK(hipMemcpyAsync(chi_d.get(), c_hi.data(), ntau * sizeof(double), hipMemcpyHostToDevice, st));
        ADMM_HIP_CHECK(hipMemcpyAsync(clo_d.get(), c_lo.data(), ntau * sizeof(double), hipMemcpyHostToDevice, st));
        ADMM_HIP_CHECK(hipMemcpyAsync(dlt_d.get(), dlt.data(), ntau * sizeof(double), hipMemcpyHostToDevice, st));
        ADMM_HIP_CHECK(hipMemcpyAsync(batch.get(), hb.data(), hb.size() * sizeof(GemvTArgs<double>), hipMemcpyHostToDevice, st));
        ADMM_HIP_CHECK(hipStreamSynchronize(st));                // (the host vectors above are read by the copies)

        const int nwg_head = std::max(1, std::min(device_info().num_cu, (n + kDenseThreads - 1) / kDenseThreads));
        const double* spart0 = b + o_g;
        double* cpart0 = b + o_c;
        auto launch_rows = [&](int par) {
            bool found = false;
            with_constant<0, kProxKindCount - 1>(kind, [&](auto kc) {
                with_constant<1, kLadMaxNpt>(lad_npt(ldxt), [&](auto npt) {
                    constexpr int K = decltype(kc)::value, N = decltype(npt)::value;
                    found = with_constant<2, kProxKinds[K].max_slots[N - 1]>(nslots, [&](auto ns) {
                        hipLaunchKernelGGL((quant_rows_kernel<N, decltype(ns)::value, K>), dim3(lad_nwg), dim3(kLadThreads), 0, st, q, (long long)stride, chi_d.get(), clo_d.get(), par,
                                           Xt.get(), ldxt, spart0, g2.pl.nseg, g2.stride, cpart0, lad_rows, (const double*)dlt_d.get());
                    });
                });
            });
            if (!found) throw Error(ADMM_ERR_INTERNAL, "slotted grid: no rows kernel for this layout");
        };
        const long long bound = (long long)ntau * ((long long)opts.maxit + 2);      // (all quantiles through one slot)
        LoopTimes lt = run_until_done(st, (const int*)ints.get(), batch_iters((int)opt_int(Opt::BATCH_ITERS, 0), 8), bound, [&](long long g) {
            const int par = (int)(g & 1);
            if (kProxKinds[kind].enet) hipLaunchKernelGGL(quant_head_kernel<QuantGridZ>, dim3(nwg_head, nslots), dim3(kDenseThreads), (size_t)lad_nwg * 8 * sizeof(double), st, q, G, par);
            else hipLaunchKernelGGL(quant_head_kernel<QuantGrid>, dim3(nwg_head, nslots), dim3(kDenseThreads), (size_t)lad_nwg * 8 * sizeof(double), st, q, (QuantGrid)G, par);
            launch_gemv_t_batch<double>(batch.get(), nslots, g2.pl.grid, g2.pl.lds_bytes, g2.pl.nt, st);
            launch_rows(par);
        });
        S.t_loop += lt.wall_s; S.loop_ms_events += lt.events_ms; S.xupdate_launches += lt.launched;
        read_back(hi.data(), ints.get(), hi.size() * sizeof(int), st);
        std::vector<double> hr(ntau);
        read_back(hr.data(), rho_fin.get(), ntau * sizeof(double), st);
        for (int k = 0; k < ntau; ++k) {
            niter[k] = hi[3 + nslots + k];
            S.total_iter += niter[k];
            coef_of(fin.get() + (size_t)k * ldn, coef + (size_t)k * p);
        }
        if (zpen != nullptr) read_back(zpen, zpen_d.get(), (size_t)ntau * ridge_p0 * sizeof(double), st);
        S.rho = hr[ntau - 1];
        S.xupdate_variant = 8 + nslots;
    }
};

}  // namespace

void solve_lad(const DeviceData<double>& d, const admm_opts& opts, DenseResult& res, hipStream_t st) {
    const int p = d.p;
    LadProblem P(d, opts, st);
    P.setup(res.stats);
    std::vector<double> coef(p), out(p);
    res.niter = P.loop(LadProx{}, res, coef.data());
    double b0 = 0;
    recover_coef<double>(d, coef.data(), &b0, out.data());      // LAD.cpp:41
    res.beta.assign(p + 1, 0.0);
    res.beta[0] = b0;
    for (int j = 0; j < p; ++j) res.beta[j + 1] = out[j];
}

// ---------------------------------------------------------------------------------------------- quantile regression
__global__ void __launch_bounds__(256) ones_column_kernel(double* col, int n, long long ld) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < ld) col[i] = i < n ? 1.0 : 0.0;
}
// X | 1: the fitted intercept's column behind the standardised matrix; d.p counts it from here on
static void append_ones_column(DeviceData<double>& d, hipStream_t st) {
    const int p0 = d.p;
    DevBuf<double> X1((size_t)d.ldx * (p0 + 1));
    ADMM_HIP_CHECK(hipMemcpyAsync(X1.get(), d.X.get(), (size_t)d.ldx * p0 * sizeof(double), hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(ones_column_kernel, dim3((unsigned)((d.ldx + 255) / 256)), dim3(256), 0, st, X1.get() + (size_t)d.ldx * p0, d.n, d.ldx);
    ADMM_HIP_CHECK(hipStreamSynchronize(st));
    d.X = std::move(X1);
    d.p = p0 + 1;
}

// p0 more rows behind the n of X (all columns, the ones column included) and of the response, zero: the ridge rows sqrt(lambda) e_j', whose
// p0 non-zeros LadProblem::setup_lambda writes per lambda.  d.n counts them from here on; the leading dimension grows with it.
static void append_ridge_rows(DeviceData<double>& d, int p0, hipStream_t st) {
    const int n0 = d.n;
    const long long ld1 = round_up((long long)n0 + p0, 32);
    DevBuf<double> X1((size_t)ld1 * d.p), Y1((size_t)ld1);
    X1.zero(st); Y1.zero(st);
    for (int c0 = 0; c0 < d.p; c0 += 65535) {                    // (the grid's y extent)
        const int nc = std::min(65535, d.p - c0);
        hipLaunchKernelGGL(copy_cols_f64_kernel, dim3((n0 + 255) / 256, nc), dim3(256), 0, st, d.X.get() + (size_t)c0 * d.ldx, d.ldx, n0, X1.get() + (size_t)c0 * ld1, ld1);
    }
    ADMM_HIP_CHECK(hipStreamSynchronize(st));
    d.X = std::move(X1);
    d.Y = std::move(Y1);
    d.ldx = ld1;
    d.n = n0 + p0;
}

// d: the standardised data (DataStd flag 3 with the intercept, 1 without); with the intercept the loop fits one more column of ones.
// fits: the grid in the units of the standardised response, all of one prox kind.  What admm_hip_quantreg and admm_hip_huber share:
// the ones column, the setup, the choice of slots, the loops and the recovery.
static void run_lad_fits(LadProblem& P, DeviceData<double>& d, int p0, bool intercept, const std::vector<LadProx>& fits, QuantResult& res, std::vector<double>* coef_std = nullptr);
static void solve_lad_grid(DeviceData<double>& d, bool intercept, const admm_opts& opts, const std::vector<LadProx>& fits, QuantResult& res, hipStream_t st) {
    const int p0 = d.p;
    if (intercept) append_ones_column(d, st);
    LadProblem P(d, opts, st);
    P.setup(res.dense.stats);
    run_lad_fits(P, d, p0, intercept, fits, res);
}
// the fits of a grid on a problem that is set up (d.p: the loop's columns, p0 of them the user's): the choice of slots, the loops, the recovery.
// coef_std: if given, takes the fits' coefficients on the loop's own (standardised) columns, [fit][d.p], as the recovery reads them.
static void run_lad_fits(LadProblem& P, DeviceData<double>& d, int p0, bool intercept, const std::vector<LadProx>& fits, QuantResult& res, std::vector<double>* coef_std) {
    const int ntau = (int)fits.size();
    const int n = d.n, p = d.p;
    DenseResult& dr = res.dense;

    // slots: the one-pass branch only; QUANT_SLOTS 0 = automatic, 1 = serial, 2 .. 8 = at most that many, clipped to what the registers
    // of the shape's layout hold and to the number of quantiles.  The get_x vectors of all quantiles (n x ntau) must fit beside the problem.
    int slots = 1;
    if (P.onepass && dr.trace_cap == 0 && ntau >= 2) {
        const long long want = opt_int(Opt::QUANT_SLOTS, 0);
        const ProxKind& K = kProxKinds[fits[0].kind];
        slots = std::min(std::min(want == 0 ? K.auto_slots : (int)want, K.max_slots[lad_npt(P.ldxt) - 1]), ntau);
        if ((size_t)ntau * (size_t)n * sizeof(double) > (size_t(2) << 30)) slots = 1;
    }
    std::vector<double> coef((size_t)ntau * p);
    res.niter.assign(ntau, 0);
    // kProxLogitE / kProxPoisE: the penalised coefficients are read from the penalty rows of the last z (exact zeros), b_j = z_{n0 + j} / c with c the
    // rows' scale sqrt(n0); get_x keeps only the intercept's entry
    const bool enet = kProxKinds[fits[0].kind].enet;
    std::vector<double> zpen(enet ? (size_t)ntau * p0 : 0);
    if (slots >= 2) {
        P.loop_slots(slots, fits, dr.stats, res.niter.data(), coef.data(), enet ? zpen.data() : nullptr);
    } else {
        for (int k = 0; k < ntau; ++k) res.niter[k] = P.loop(fits[k], dr, coef.data() + (size_t)k * p, enet ? zpen.data() + (size_t)k * p0 : nullptr);
    }
    if (enet) {
        const double c = std::sqrt((double)P.n0);
        for (int k = 0; k < ntau; ++k)
            for (int j = 0; j < p0; ++j) coef[(size_t)k * p + j] = zpen[(size_t)k * p0 + j] / c;
    }
    dr.niter = res.niter[0];
    // beta_j = b_j scaleY / scaleX_j;  beta_0 = (meanY - sum beta_j meanX_j) + scaleY b_{p+1}
    res.beta.assign((size_t)(p0 + 1) * ntau, 0.0);
    d.p = p0;                                                    // (recover_coef: the user's columns)
    std::vector<double> out(p0);
    for (int k = 0; k < ntau; ++k) {
        const double* b = coef.data() + (size_t)k * p;
        double b0 = 0;
        recover_coef<double>(d, b, &b0, out.data());
        if (intercept) b0 = b0 + d.scaleY * b[p0];
        double* col = res.beta.data() + (size_t)k * (p0 + 1);
        col[0] = b0;
        for (int j = 0; j < p0; ++j) col[j + 1] = out[j];
    }
    d.p = p;
    if (coef_std != nullptr) *coef_std = std::move(coef);
}

void solve_quantreg(DeviceData<double>& d, bool intercept, const admm_opts& opts, const double* tau, int ntau, QuantResult& res, hipStream_t st) {
    std::vector<LadProx> fits(ntau);
    for (int k = 0; k < ntau; ++k) { fits[k].c_hi = 2.0 * (1.0 - tau[k]); fits[k].c_lo = 2.0 * tau[k]; }
    solve_lad_grid(d, intercept, opts, fits, res, st);
}

// Huber / expectile regression: the same grid with the Huber form of the prox.  delta is the caller's, in the units of y; the loop runs
// on y / scaleY and H is positively homogeneous in (r, delta), so it uses delta / scaleY (+inf stays +inf).
void solve_huber(DeviceData<double>& d, bool intercept, const admm_opts& opts, const double* delta, const double* tau, int nfit, QuantResult& res, hipStream_t st) {
    std::vector<LadProx> fits(nfit);
    for (int k = 0; k < nfit; ++k) {
        fits[k].kind = kProxHuber;
        fits[k].c_hi = 2.0 * (1.0 - tau[k]); fits[k].c_lo = 2.0 * tau[k];
        fits[k].delta = delta[k] / d.scaleY;
    }
    solve_lad_grid(d, intercept, opts, fits, res, st);
}

// ---------------------------------------------------------------------------------------------- logistic regression
// counts[0]: labels that are neither 0.0 nor 1.0 (NaN included); counts[1]: the ones
__global__ void __launch_bounds__(256) logit_count_labels_kernel(const double* __restrict__ y, int n, unsigned long long* counts) {
    unsigned bad = 0, ones = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const double v = y[i];
        if (v == 1.0) ++ones;
        else if (!(v == 0.0)) ++bad;
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) { bad += __shfl_xor(bad, m, 64); ones += __shfl_xor(ones, m, 64); }
    if ((threadIdx.x & 63) == 0) {
        if (bad) atomicAdd(&counts[0], (unsigned long long)bad);
        if (ones) atomicAdd(&counts[1], (unsigned long long)ones);
    }
}
void logit_count_labels(const double* y_dev, int n, long long* bad, long long* ones, hipStream_t st) {
    DevBuf<unsigned long long> c(2);
    c.zero(st);
    hipLaunchKernelGGL(logit_count_labels_kernel, dim3(std::max(1, std::min(1024, (n + 255) / 256))), dim3(256), 0, st, y_dev, n, c.get());
    unsigned long long h[2];
    read_back(h, c.get(), sizeof(h), st);
    *bad = (long long)h[0]; *ones = (long long)h[1];
}
// s_i = 2 y_i - 1, and row i of the column-major X (the ones column included) times s_i
__global__ void __launch_bounds__(256) logit_signs_kernel(const double* __restrict__ y, int n, double* __restrict__ s) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) s[i] = y[i] == 1.0 ? 1.0 : -1.0;
}
__global__ void __launch_bounds__(256) logit_fold_kernel(double* __restrict__ X, long long ldx, int n, int p, const double* __restrict__ s) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const double sr = s[r];
    for (int c = blockIdx.y; c < p; c += gridDim.y) X[(size_t)c * ldx + r] *= sr;
}

// Logistic regression: min sum log(1 + exp(-s_i (b0 + x_i'b))), s = 2 y - 1, as the LAD loop on X~ = diag(s) [X | 1] with a ZERO response
// and the prox of log(1 + e^-z) (logit2).  X~'X~ = [X 1]'[X 1], so setup, branches, control and get_x are LAD's; the response is not a
// scale: recovery with scaleY = 1, meanY = 0.  y_dev: the caller's labels (validated: 0.0 / 1.0, both present) on the device.
void solve_logit(DeviceData<double>& d, bool intercept, const double* y_dev, const admm_opts& opts, DenseResult& res, hipStream_t st) {
    const int n = d.n, p0 = d.p;
    if (intercept) append_ones_column(d, st);
    const int p = d.p;
    DevBuf<double> sgn(n);
    hipLaunchKernelGGL(logit_signs_kernel, dim3((n + 255) / 256), dim3(256), 0, st, y_dev, n, sgn.get());
    hipLaunchKernelGGL(logit_fold_kernel, dim3((n + 255) / 256, std::min(p, 65535)), dim3(256), 0, st, d.X.get(), d.ldx, n, p, sgn.get());
    d.Y.zero(st);
    d.scaleY = 1.0; d.meanY = 0.0;
    LadProblem P(d, opts, st);
    P.setup(res.stats);
    LadProx px;
    px.kind = kProxLogit; px.signs = sgn.get();
    std::vector<double> coef(p), out(p0);
    res.niter = P.loop(px, res, coef.data());
    d.p = p0;                                                    // (recover_coef: the user's columns)
    double b0 = 0;
    recover_coef<double>(d, coef.data(), &b0, out.data());
    d.p = p;
    if (intercept) b0 = b0 + coef[p0];
    res.beta.assign(p0 + 1, 0.0);
    res.beta[0] = b0;
    for (int j = 0; j < p0; ++j) res.beta[j + 1] = out[j];
}

// column c of the n x ncol labels (leading dimension n) as signs, leading dimension lds; the padding rows zero
__global__ void __launch_bounds__(256) logit_sign_matrix_kernel(const double* __restrict__ y, int n, int ncol, long long lds, double* __restrict__ s) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= lds) return;
    for (int c = blockIdx.y; c < ncol; c += gridDim.y) s[(size_t)c * lds + i] = i < n ? (y[(size_t)c * n + i] == 1.0 ? 1.0 : -1.0) : 0.0;
}

// Logistic regression for ncol label columns on ONE setup (admm_hip_logit_multi).  Nothing is folded: the loop runs on [X_std | 1] with a
// zero response and the prox takes row i's sign s_i = 2 y_i - 1 itself (kProxLogitS), so the matrix, its Gram, the inverse, the transpose
// and the hat matrix are shared by all columns, and on the one-pass branch several columns advance on one pass over X: solve_lad_grid
// with the signs as the grid.  Column k equals solve_logit on that column -- every n-vector is s times the folded loop's, everything else
// identical, rounding being symmetric in sign.  y_dev: n x ncol validated labels on the device, leading dimension n.
void solve_logit_multi(DeviceData<double>& d, bool intercept, const double* y_dev, int ncol, const admm_opts& opts, QuantResult& res, hipStream_t st) {
    const int n = d.n;
    const long long lds = round_up(n, 32);
    DevBuf<double> sgn((size_t)lds * ncol);
    hipLaunchKernelGGL(logit_sign_matrix_kernel, dim3((unsigned)((lds + 255) / 256), std::min(ncol, 65535)), dim3(256), 0, st, y_dev, n, ncol, lds, sgn.get());
    d.Y.zero(st);
    d.scaleY = 1.0; d.meanY = 0.0;
    std::vector<LadProx> fits(ncol);
    for (int k = 0; k < ncol; ++k) { fits[k].kind = kProxLogitS; fits[k].signs = sgn.get() + (size_t)k * lds; }
    solve_lad_grid(d, intercept, opts, fits, res, st);
}

// What the fits with penalty rows share ahead of their setup: the ones column, the p0 zero rows behind the data, the tag matrix (signs or
// counts: `tags` writes column c of the n0 x ncol labels with leading dimension round_up(d.n, 32) and its own filler behind them), and
// a response that is no scale.  Returns the tag matrix.
using TagMatrixKernel = void (*)(const double*, int, int, long long, double*);
static void augment_rows(DeviceData<double>& d, bool intercept, hipStream_t st) {
    const int p0 = d.p;
    if (intercept) append_ones_column(d, st);
    append_ridge_rows(d, p0, st);
    d.scaleY = 1.0; d.meanY = 0.0;
}
static DevBuf<double> augment_tagged(DeviceData<double>& d, bool intercept, const double* y_dev, int ncol, TagMatrixKernel tags, hipStream_t st) {
    const int n0 = d.n;
    augment_rows(d, intercept, st);
    const long long lds = round_up(d.n, 32);
    DevBuf<double> tag((size_t)lds * ncol);
    hipLaunchKernelGGL(tags, dim3((unsigned)((lds + 255) / 256), std::min(ncol, 65535)), dim3(256), 0, st, y_dev, n0, ncol, lds, tag.get());
    return tag;
}

// Ridge logistic regression (admm_hip_logit_ridge): sum log(1 + exp(-s_i (b0 + x_i'b))) + lambda / 2 sum b_j^2 per label column and
// lambda, b on the standardised scale, the intercept not penalised.  The penalty is not written on b -- the x-update's matrix would be
// X'X + (lambda / rho) D and change with rho -- but as p0 more ROWS sqrt(lambda) e_j' with a zero response and the loss z^2 / 2: the Gram
// matrix of the augmented rows is X'X + lambda D whatever rho does, and the loop is solve_logit_multi's with one more case in the prox
// (kProxLogitR: sign 0 = a square-loss row).  Once per call: the upload's standardisation, the ones column, the ridge rows, the Gram
// matrix of the data rows, the transpose, the sign matrix.  Per lambda, in the order given, every fit from a cold start: M = G0 + lambda
// D, the ridge rows' entries, the inverse (and the hat matrix), then the ncol columns as solve_lad_grid runs a grid.
// res.beta: (p + 1) x ncol x nlambda, res.niter: ncol x nlambda.
void solve_logit_ridge(DeviceData<double>& d, bool intercept, const double* y_dev, int ncol, const double* lambda, int nlambda, const admm_opts& opts, QuantResult& res,
                       hipStream_t st) {
    const int n0 = d.n, p0 = d.p;
    const DevBuf<double> sgn = augment_tagged(d, intercept, y_dev, ncol, logit_sign_matrix_kernel, st);
    const long long lds = round_up(d.n, 32);
    std::vector<LadProx> fits(ncol);
    for (int k = 0; k < ncol; ++k) { fits[k].kind = kProxLogitR; fits[k].signs = sgn.get() + (size_t)k * lds; }
    LadProblem P(d, opts, st);
    P.setup_ridge(n0, p0, res.dense.stats);
    res.beta.clear(); res.niter.clear();
    for (int l = 0; l < nlambda; ++l) {
        P.setup_lambda(lambda[l], res.dense.stats);
        QuantResult one;
        one.dense.trace_cap = res.dense.trace_cap; one.dense.state_cap = res.dense.state_cap;
        one.dense.stats = res.dense.stats;
        run_lad_fits(P, d, p0, intercept, fits, one);
        res.beta.insert(res.beta.end(), one.beta.begin(), one.beta.end());
        res.niter.insert(res.niter.end(), one.niter.begin(), one.niter.end());
        res.dense.stats = one.dense.stats;
        if (l == nlambda - 1) {
            res.dense.niter = one.dense.niter;
            res.dense.trace = std::move(one.dense.trace); res.dense.state = std::move(one.dense.state); res.dense.state_dim = one.dense.state_dim;
        }
    }
}

// Elastic-net logistic regression (admm_hip_logit_enet): per label column and cell (lambda, alpha)
//     sum log(1 + exp(-s_i (b0 + x_i'b))) + lambda (alpha sum |b_j| + (1 - alpha) / 2 sum b_j^2),
// b on the standardised scale, the intercept not penalised.  solve_logit_ridge's restatement with the penalty's constants moved from
// the rows into the prox: the p0 penalty rows are c e_j' for EVERY cell, z_{n0 + j} = c b_j, and their loss is
// (lambda alpha / c) |z| + (lambda (1 - alpha) / c^2) z^2 / 2 (kProxLogitE: c_hi, c_lo).  The Gram matrix of the augmented rows is
// X'X + c^2 D whatever lambda, alpha and rho are: ONE Gram matrix, ONE inverse (and hat matrix), ONE transpose per call, and every cell
// of the ncol x ncell grid is one more fit of run_lad_fits -- cell-major, fit cell * ncol + column --, so the slots refill across the
// whole grid.  c^2 = n0, the squared norm of a standardised column: with unit rows the loop needs hundreds to thousands of iterations,
// with c = sqrt(n0) 18 - 66 (tests/test_logit_enet_host.py).  Returned: the penalty rows of the last z over c (exact zeros), the
// intercept from get_x (run_lad_fits).  res.beta: (p + 1) x ncol x ncell, res.niter: ncol x ncell.
// (solve_poisson is the same function with another kind and another tag matrix: solve_enet_rows.)
//
// Cross-validation (folds != NULL: admm_hip_logit_enet_cv, admm_hip_poisson_cv).  A held-out row is a row whose loss is zero, and the
// prox of the zero function is the identity (row_prox_tagged's held-out tags): with it a fold's fit on the FULL augmented matrix is the
// training rows' problem -- the held-out rows' duals vanish after the first iteration and leave the residuals.  So the matrix, its
// Gram, the inverse, the hat matrix and the transpose are the full-data call's, formed once, and the folds are more COLUMNS of the tag
// matrix: column s ncol + c is label (count) column c with the rows of slot s's fold tagged held out -- slot 0 holds out nothing (the
// full-data fit), slot s >= 1 fold s - 1.  The fits run cell-major, then slot, then column, fit (cell nslot + s) ncol + c, so the
// slotted head's fit mod sgn_cols is the fit's tag column.  folds->single >= -1: one slot only, holding out that fold (-1: none).
// fold_dev, if given: the held-out deviance of every (fold, cell, column), glm_cv_deviance below.
template <bool POIS>
__global__ void __launch_bounds__(256) fold_tag_matrix_kernel(const double* __restrict__ y, int n, int ncol, int ntag, long long lds, const int* __restrict__ fold_id, int held0,
                                                              double* __restrict__ s) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= lds) return;
    const int fi = i < n ? fold_id[i] : -1;
    for (int t = blockIdx.y; t < ntag; t += gridDim.y) {
        const int c = t % ncol, held = held0 + t / ncol;             // (held -1: nothing held out)
        double v = POIS ? -1.0 : 0.0;                                // the penalty rows and the padding: as the public calls' matrices
        if (i < n) {
            const double yv = y[(size_t)c * n + i];
            v = held >= 0 && fi == held ? (POIS ? kHeldOutPoisE : kHeldOutLogitE) : (POIS ? yv : (yv == 1.0 ? 1.0 : -1.0));
        }
        s[(size_t)t * lds + i] = v;
    }
}

// Held-out deviance, in double and the same bits on every run: no atomics, every sum in one fixed order.
// Rows kernel: one wave per data row, in the order `perm` (the rows sorted by fold, stably); lane = one (cell, column) pair, 64 pairs
// at a time.  eta = the row of the stored transpose (the standardised columns and the ones column: no second copy of X) times the
// standardised coefficients of the fit (cell, the ROW's fold, column), which the host lays out as B[fold][column j][pair] so that a
// wave's loads are contiguous; the row's entries are wave-uniform.  One multiply-add per column, j ascending.  A row is read by one
// wave, once per 64 pairs.  rowdev: [position in perm][pair].
template <bool POIS>
__global__ void __launch_bounds__(256) glm_cv_rowdev_kernel(const double* __restrict__ Xt, long long ldxt, int p, int n, const int* __restrict__ perm,
                                                            const int* __restrict__ fold_id, const double* __restrict__ B, int npair, int ncol,
                                                            const double* __restrict__ y, double* __restrict__ rowdev) {
    const int lane = threadIdx.x & 63;
    const long long pos = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pos >= n) return;
    const int i = perm[pos], f = fold_id[i];
    const double* xr = Xt + (size_t)i * ldxt;
    for (int pair0 = 0; pair0 < npair; pair0 += 64) {
        const int pair = pair0 + lane;
        if (pair >= npair) break;
        const double* b = B + (size_t)f * p * npair + pair;
        double eta = 0.0;
        for (int j = 0; j < p; ++j) eta = fma(xr[j], b[(size_t)j * npair], eta);
        const double yv = y[(size_t)(pair % ncol) * n + i];
        double dev;
        if (POIS) {
            const double mu = exp(eta);
            dev = 2.0 * ((yv > 0.0 ? yv * log(yv / mu) : 0.0) - (yv - mu));
        } else {
            const double se = yv == 1.0 ? eta : -eta;                // s eta, s = 2 y - 1
            dev = 2.0 * (fmax(-se, 0.0) + log1p(exp(-fabs(eta))));
        }
        rowdev[(size_t)pos * npair + pair] = dev;
    }
}
// block (pair, f): the mean of rowdev over the positions [off[f], off[f + 1]) of fold f -- thread t adds its positions t, t + 256, ...
// in order, the 256 sums meet in a fixed tree
__global__ void __launch_bounds__(256) glm_cv_fold_mean_kernel(const double* __restrict__ rowdev, int npair, const int* __restrict__ off, double* __restrict__ out) {
    __shared__ double m[256];
    const int pair = blockIdx.x, f = blockIdx.y;
    const int lo = off[f], hi = off[f + 1];
    double s = 0.0;
    for (int q = lo + (int)threadIdx.x; q < hi; q += 256) s += rowdev[(size_t)q * npair + pair];
    m[threadIdx.x] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) m[threadIdx.x] += m[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[(size_t)f * npair + pair] = m[0] / (double)(hi - lo);
}
// fold_dev[(f ncell + l) ncol + c] = the mean deviance of fold f's rows under the fit (cell l, slot f + 1, column c).  coef: the fits'
// standardised coefficients [fit][p] (run_lad_fits), p = the loop's columns; fid: the n0 fold ids on the host, fid_dev: on the device.
static void glm_cv_deviance(bool pois, const LadProblem& P, int p, int n0, const double* y_dev, int ncol, int ncell, const std::vector<int>& fid, const int* fid_dev, int nfolds,
                            const std::vector<double>& coef, std::vector<double>& fold_dev, hipStream_t st) {
    const int npair = ncol * ncell, nslot = nfolds + 1;
    std::vector<int> off(nfolds + 1, 0), perm(n0);
    for (int i = 0; i < n0; ++i) ++off[fid[i] + 1];
    for (int f = 0; f < nfolds; ++f) off[f + 1] += off[f];
    { std::vector<int> at(off.begin(), off.end() - 1); for (int i = 0; i < n0; ++i) perm[at[fid[i]]++] = i; }
    std::vector<double> hB((size_t)nfolds * p * npair);
    for (int f = 0; f < nfolds; ++f)
        for (int l = 0; l < ncell; ++l)
            for (int c = 0; c < ncol; ++c) {
                const double* b = coef.data() + (((size_t)l * nslot + f + 1) * ncol + c) * p;
                for (int j = 0; j < p; ++j) hB[((size_t)f * p + j) * npair + (size_t)l * ncol + c] = b[j];
            }
    DevBuf<double> B(hB.size()), rowdev((size_t)n0 * npair), out((size_t)nfolds * npair);
    DevBuf<int> perm_d(n0), off_d(nfolds + 1);
    ADMM_HIP_CHECK(hipMemcpyAsync(B.get(), hB.data(), hB.size() * sizeof(double), hipMemcpyHostToDevice, st));
    ADMM_HIP_CHECK(hipMemcpyAsync(perm_d.get(), perm.data(), perm.size() * sizeof(int), hipMemcpyHostToDevice, st));
    ADMM_HIP_CHECK(hipMemcpyAsync(off_d.get(), off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice, st));
    const dim3 grid((unsigned)((n0 + 3) / 4));
    if (pois) hipLaunchKernelGGL(glm_cv_rowdev_kernel<true>, grid, dim3(256), 0, st, P.Xt.get(), P.ldxt, p, n0, perm_d.get(), fid_dev, B.get(), npair, ncol, y_dev, rowdev.get());
    else hipLaunchKernelGGL(glm_cv_rowdev_kernel<false>, grid, dim3(256), 0, st, P.Xt.get(), P.ldxt, p, n0, perm_d.get(), fid_dev, B.get(), npair, ncol, y_dev, rowdev.get());
    for (int f0 = 0; f0 < nfolds; f0 += 65535)                   // (the grid's y extent)
        hipLaunchKernelGGL(glm_cv_fold_mean_kernel, dim3(npair, std::min(65535, nfolds - f0)), dim3(256), 0, st, rowdev.get(), npair, off_d.get() + f0, out.get() + (size_t)f0 * npair);
    ADMM_HIP_CHECK(hipGetLastError());
    fold_dev.assign((size_t)nfolds * npair, 0.0);
    read_back(fold_dev.data(), out.get(), fold_dev.size() * sizeof(double), st);
}

static void solve_enet_rows(int kind, TagMatrixKernel tags, DeviceData<double>& d, bool intercept, const double* y_dev, int ncol, const double* lambda, const double* alpha,
                            int ncell, const admm_opts& opts, QuantResult& res, hipStream_t st, const GlmFolds* folds = nullptr, std::vector<double>* fold_dev = nullptr) {
    const int n0 = d.n, p0 = d.p;
    const bool pois = kind == kProxPoisE;
    const int nslot = folds == nullptr || folds->single >= -1 ? 1 : folds->nfolds + 1;
    const int ntag = ncol * nslot;
    DevBuf<double> tag;
    DevBuf<int> fid_d;
    if (folds == nullptr) {
        tag = augment_tagged(d, intercept, y_dev, ncol, tags, st);
    } else {
        augment_rows(d, intercept, st);
        fid_d.alloc(n0);
        ADMM_HIP_CHECK(hipMemcpyAsync(fid_d.get(), folds->id->data(), (size_t)n0 * sizeof(int), hipMemcpyHostToDevice, st));
        const long long ldt = round_up(d.n, 32);
        tag.alloc((size_t)ldt * ntag);
        const dim3 grid((unsigned)((ldt + 255) / 256), std::min(ntag, 65535));
        const int held0 = nslot == 1 ? folds->single : -1;
        if (pois) hipLaunchKernelGGL(fold_tag_matrix_kernel<true>, grid, dim3(256), 0, st, y_dev, n0, ncol, ntag, ldt, fid_d.get(), held0, tag.get());
        else hipLaunchKernelGGL(fold_tag_matrix_kernel<false>, grid, dim3(256), 0, st, y_dev, n0, ncol, ntag, ldt, fid_d.get(), held0, tag.get());
    }
    const long long lds = round_up(d.n, 32);
    const double c2 = (double)n0, c = std::sqrt(c2);
    std::vector<int> live;                                       // per slot: the rows of the loop less the held-out ones
    if (folds != nullptr) {
        std::vector<int> cnt(folds->nfolds, 0);
        for (int i = 0; i < n0; ++i) ++cnt[(*folds->id)[i]];
        for (int s = 0; s < nslot; ++s) {
            const int held = nslot == 1 ? folds->single : s - 1;
            live.push_back(d.n - (held >= 0 ? cnt[held] : 0));
        }
    }
    std::vector<LadProx> fits((size_t)ntag * ncell);
    for (int l = 0; l < ncell; ++l)
        for (int k = 0; k < ntag; ++k) {
            LadProx& f = fits[(size_t)l * ntag + k];
            f.kind = kind; f.ncols = ntag;
            if (folds != nullptr) f.live_rows = live[k / ncol];
            f.signs = tag.get() + (size_t)k * lds;
            f.c_hi = lambda[l] * alpha[l] / c;
            f.c_lo = lambda[l] * (1.0 - alpha[l]) / c2;
        }
    LadProblem P(d, opts, st);
    P.setup_ridge(n0, p0, res.dense.stats);
    P.setup_lambda(c2, res.dense.stats);
    std::vector<double> coef;
    run_lad_fits(P, d, p0, intercept, fits, res, fold_dev != nullptr ? &coef : nullptr);
    if (fold_dev != nullptr) glm_cv_deviance(pois, P, d.p, n0, y_dev, ncol, ncell, *folds->id, fid_d.get(), folds->nfolds, coef, *fold_dev, st);
}
void solve_glm_cv(bool pois, DeviceData<double>& d, bool intercept, const double* y_dev, int ncol, const GlmFolds& folds, const double* lambda, const double* alpha, int ncell,
                  const admm_opts& opts, QuantResult& res, std::vector<double>* fold_dev, hipStream_t st) {
    solve_enet_rows(pois ? kProxPoisE : kProxLogitE, nullptr, d, intercept, y_dev, ncol, lambda, alpha, ncell, opts, res, st, &folds, folds.single >= -1 ? nullptr : fold_dev);
}
void solve_logit_enet(DeviceData<double>& d, bool intercept, const double* y_dev, int ncol, const double* lambda, const double* alpha, int ncell, const admm_opts& opts,
                      QuantResult& res, hipStream_t st) {
    solve_enet_rows(kProxLogitE, logit_sign_matrix_kernel, d, intercept, y_dev, ncol, lambda, alpha, ncell, opts, res, st);
}

// lambda_1 of admm_hip_logit_enet_lambda_max: per label column max_j |x~_j'r|, r = y - mean(y) (mean[c] = 0.5 without the intercept)
__global__ void __launch_bounds__(256) enet_resid_kernel(const double* __restrict__ y, int n, int ncol, long long ldr, const double* __restrict__ mean, double* __restrict__ r) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= ldr) return;
    for (int c = blockIdx.y; c < ncol; c += gridDim.y) r[(size_t)c * ldr + i] = i < n ? y[(size_t)c * n + i] - mean[c] : 0.0;
}
// block c: the nseg partial rows of product c summed in order, then the largest magnitude over the p outputs
__global__ void __launch_bounds__(256) enet_lambda_one_kernel(const double* __restrict__ part, long long pstride, int nseg, long long ostride, int p, double* __restrict__ out) {
    __shared__ double m[256];
    const double* pc = part + (size_t)blockIdx.x * pstride;
    double best = 0.0;
    for (int j = threadIdx.x; j < p; j += 256) {
        double s = 0.0;
        for (int g = 0; g < nseg; ++g) s += pc[(size_t)g * ostride + j];
        best = fmax(best, fabs(s));
    }
    m[threadIdx.x] = best;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) m[threadIdx.x] = fmax(m[threadIdx.x], m[threadIdx.x + h]);
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = m[0];
}
// d: the standardised data BEFORE the ones column; mean: ncol host values; out: ncol host values.  One batched gemv_t launch for the
// ncol right-hand sides (at most 65535 per launch).
void logit_enet_lambda_one(const DeviceData<double>& d, const double* y_dev, int ncol, const double* mean, double* out, hipStream_t st) {
    const int n = d.n, p = d.p;
    const long long ldr = round_up(n, 32);
    GemvT<double> g;
    g.init(d.X.get(), d.ldx, n, p);
    const size_t pstride = (size_t)g.pl.nseg * g.stride;
    DevBuf<double> r((size_t)ldr * ncol), part(pstride * ncol), mean_d(ncol), out_d(ncol);
    ADMM_HIP_CHECK(hipMemcpyAsync(mean_d.get(), mean, (size_t)ncol * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(enet_resid_kernel, dim3((unsigned)((ldr + 255) / 256), std::min(ncol, 65535)), dim3(256), 0, st, y_dev, n, ncol, ldr, mean_d.get(), r.get());
    std::vector<GemvTArgs<double>> hb(ncol);
    for (int c = 0; c < ncol; ++c) {
        hb[c] = g.args_partials(r.get() + (size_t)c * ldr, nullptr);
        hb[c].out[0] = part.get() + (size_t)c * pstride;
    }
    DevBuf<GemvTArgs<double>> batch(ncol);
    ADMM_HIP_CHECK(hipMemcpyAsync(batch.get(), hb.data(), hb.size() * sizeof(GemvTArgs<double>), hipMemcpyHostToDevice, st));
    for (int c0 = 0; c0 < ncol; c0 += 65535)
        launch_gemv_t_batch<double>(batch.get() + c0, std::min(65535, ncol - c0), g.pl.grid, g.pl.lds_bytes, g.pl.nt, st);
    hipLaunchKernelGGL(enet_lambda_one_kernel, dim3(ncol), dim3(256), 0, st, part.get(), (long long)pstride, g.pl.nseg, g.stride, p, out_d.get());
    read_back(out, out_d.get(), (size_t)ncol * sizeof(double), st);
}

// ---------------------------------------------------------------------------------------------- Poisson regression
// block c: column c of the n x ncol counts -- stats[2 c] = the entries that are not finite or lie below zero, stats[2 c + 1] = the
// column's sum (the waves' sums added in wave order: the same on every run)
__global__ void __launch_bounds__(256) pois_column_stats_kernel(const double* __restrict__ y, int n, double* __restrict__ stats) {
    __shared__ double scratch[2 * 4];
    const double* yc = y + (size_t)blockIdx.x * n;
    double acc[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < n; i += 256) {
        const double v = yc[i];
        if (!(v >= 0.0) || isinf(v)) acc[0] += 1.0;
        else acc[1] += v;
    }
    block_sum<double, 2>(acc, scratch);
    if (threadIdx.x == 0) { stats[2 * blockIdx.x] = acc[0]; stats[2 * blockIdx.x + 1] = acc[1]; }
}
// bad: the entries of ALL columns that are not finite or negative; sums: ncol host values (of the valid entries)
void pois_column_stats(const double* y_dev, int n, int ncol, long long* bad, double* sums, hipStream_t st) {
    DevBuf<double> s_d((size_t)2 * ncol);
    std::vector<double> h((size_t)2 * ncol);
    for (int c0 = 0; c0 < ncol; c0 += 65535) {
        const int nc = std::min(65535, ncol - c0);
        hipLaunchKernelGGL(pois_column_stats_kernel, dim3(nc), dim3(256), 0, st, y_dev + (size_t)c0 * n, n, s_d.get() + (size_t)2 * c0);
    }
    read_back(h.data(), s_d.get(), h.size() * sizeof(double), st);
    *bad = 0;
    for (int c = 0; c < ncol; ++c) { *bad += (long long)h[2 * c]; sums[c] = h[2 * c + 1]; }
}
// column c of the n x ncol counts (leading dimension n) with leading dimension lds; the rows behind the n data rows -- the penalty rows
// and the padding -- carry the marker -1.0 (kProxPoisE)
__global__ void __launch_bounds__(256) pois_count_matrix_kernel(const double* __restrict__ y, int n, int ncol, long long lds, double* __restrict__ s) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= lds) return;
    for (int c = blockIdx.y; c < ncol; c += gridDim.y) s[(size_t)c * lds + i] = i < n ? y[(size_t)c * n + i] : -1.0;
}

// Poisson regression with the elastic-net penalty (admm_hip_poisson): per count column and cell (lambda, alpha)
//     sum [exp(eta_i) - y_i eta_i] + lambda (alpha sum |b_j| + (1 - alpha) / 2 sum b_j^2),   eta_i = b0 + x_i'b,
// b on the standardised scale, the intercept not penalised.  solve_logit_enet with another loss on the data rows: the same penalty rows
// c e_j', c^2 = n0, for every cell, the same constants c_hi = lambda alpha / c, c_lo = lambda (1 - alpha) / c^2 in the prox, ONE Gram
// matrix X'X + n0 D, inverse and transpose per call, the ncol x ncell fits cell-major as one grid of run_lad_fits, the penalised
// coefficients from the penalty rows of the last z.  The count matrix stands where the sign matrix stood (kProxPoisE).  lambda = 0: both
// constants are 0 and a penalty row's prox is the identity -- the plain Poisson GLM on the same inverse.
void solve_poisson(DeviceData<double>& d, bool intercept, const double* y_dev, int ncol, const double* lambda, const double* alpha, int ncell, const admm_opts& opts,
                   QuantResult& res, hipStream_t st) {
    solve_enet_rows(kProxPoisE, pois_count_matrix_kernel, d, intercept, y_dev, ncol, lambda, alpha, ncell, opts, res, st);
}

__global__ void __launch_bounds__(256) pois_prox_hook_kernel(const double* __restrict__ v, const double* __restrict__ y, long long m, double t, double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < m) out[i] = pois2(v[i], y[i], t);
}
// test hook admm_hip_test_poisson_prox: the device prox over arrays (host in, host out)
void test_poisson_prox(const double* v, const double* y, long long m, double t, double* out) {
    Stream st;
    DevBuf<double> dv((size_t)m), dy((size_t)m), dz((size_t)m);
    ADMM_HIP_CHECK(hipMemcpyAsync(dv.get(), v, (size_t)m * sizeof(double), hipMemcpyHostToDevice, st.s));
    ADMM_HIP_CHECK(hipMemcpyAsync(dy.get(), y, (size_t)m * sizeof(double), hipMemcpyHostToDevice, st.s));
    hipLaunchKernelGGL(pois_prox_hook_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st.s, dv.get(), dy.get(), m, t, dz.get());
    read_back(out, dz.get(), (size_t)m * sizeof(double), st.s);
}

__global__ void __launch_bounds__(256) logit_prox_hook_kernel(const double* __restrict__ v, long long m, double t, double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < m) out[i] = prox2<kProxLogit>(v[i], t, t, 0.0);
}
// test hook admm_hip_test_logit_prox: the device prox over an array (host in, host out)
void test_logit_prox(const double* v, long long m, double t, double* out) {
    Stream st;
    DevBuf<double> dv((size_t)m), dz((size_t)m);
    ADMM_HIP_CHECK(hipMemcpyAsync(dv.get(), v, (size_t)m * sizeof(double), hipMemcpyHostToDevice, st.s));
    hipLaunchKernelGGL(logit_prox_hook_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st.s, dv.get(), m, t, dz.get());
    read_back(out, dz.get(), (size_t)m * sizeof(double), st.s);
}

// ---------------------------------------------------------------------------------------------- BP
void solve_bp(const DeviceData<double>& d, const admm_opts& opts, DenseResult& res, hipStream_t st) {
    const int n = d.n, p = d.p;
    admm_stats& S = res.stats;
    const long long ldn = round_up(n, 128);                // whole 128-blocks for the matrix-core factorisation

    // AA' = LL' (ADMMBP.h:167-169)
    double t0 = now_s();
    DevBuf<double> G((size_t)ldn * ldn); G.zero(st);
    gram_full<double>(d.X.get(), d.ldx, n, p, false, G.get(), ldn, st);
    ADMM_HIP_CHECK(hipStreamSynchronize(st));
    S.t_gram = now_s() - t0;
    t0 = now_s();
    // B = L^-1 A (ADMMBP.h:173-182) and its transpose; w0 = L^-1 b; cache_AAAb = B' w0 = A'(AA')^-1 b (:170)
    DevBuf<double> B((size_t)d.ldx * p);
    DevBuf<double> w0(d.ldx); w0.zero(st);
    const long long ldbt = round_up(p, 32);
    DevBuf<double> Bt((size_t)ldbt * n); Bt.zero(st);
    if (opt_is(Opt::FACTOR, "rocsolver")) {
        cholesky_lower<double>(G.get(), ldn, n, st);
        ADMM_HIP_CHECK(hipMemcpyAsync(B.get(), d.X.get(), (size_t)d.ldx * p * sizeof(double), hipMemcpyDeviceToDevice, st));
        trsm_left_lower<double>(G.get(), ldn, n, B.get(), d.ldx, p, st);
        ADMM_HIP_CHECK(hipMemcpyAsync(w0.get(), d.Y.get(), (size_t)d.ldx * sizeof(double), hipMemcpyDeviceToDevice, st));
        trsm_left_lower<double>(G.get(), ldn, n, w0.get(), d.ldx, 1, st);
        transpose<double>(B.get(), d.ldx, n, p, Bt.get(), ldbt, st);
    } else {
        // hand-written matrix-core path: blocked Cholesky fused with U = L^-T; then B' = A' U is one NT product
        // (B'[j, i] = sum_k A'[j, k] W[i, k] with W = U' = L^-1), B its transpose, w0 = U' b
        DevBuf<double> U = cholesky_linvt_mfma_f64(G.get(), ldn, n, st);
        const int nk = (int)round_up(n, 8);
        const long long ldxt = round_up(p, 128);
        DevBuf<double> Xt((size_t)ldxt * nk), W((size_t)ldn * ldn);
        Xt.zero(st);
        transpose<double>(d.X.get(), d.ldx, n, p, Xt.get(), ldxt, st);           // A' (p x n), output index contiguous
        transpose<double>(U.get(), ldn, (int)ldn, (int)ldn, W.get(), ldn, st);    // W = L^-1, zero padded
        DevBuf<double> Btp((size_t)ldxt * n);                                     // B' with whole 128-row blocks
        gemm_nt_f64(Xt.get(), ldxt, W.get(), ldn, Btp.get(), ldxt, p, n, nk, st, true);      // (W = L^-1: lower triangular, the K loop of column block j ends at its last column)
        hipLaunchKernelGGL(copy_cols_f64_kernel, dim3((p + 255) / 256, n), dim3(256), 0, st, Btp.get(), ldxt, p, Bt.get(), ldbt);
        transpose<double>(Bt.get(), ldbt, p, n, B.get(), d.ldx, st);
        GemvT<double> gU;                                                         // w0 = U' b
        gU.init(U.get(), ldn, n, n);
        gU.run(d.Y.get(), w0.get(), nullptr, st);
        ADMM_HIP_CHECK(hipStreamSynchronize(st));                                 // temporaries are released here
    }
    const long long ldp = round_up(p, 32);
    DevBuf<double> AAAb(ldp); AAAb.zero(st);
    // One-pass form (default; ADMM_HIP_BP_ONEPASS=0 keeps the two streaming products of ADMMBP.h:65-66): only B' w streams per
    // iteration, B vec comes from n-sized recurrences + a gather over the non-zeros of z (DenseParams), and the second stored
    // layout of B (its transpose, another 8np bytes) is a setup temporary.
    const bool onepass = !opt_off(Opt::BP_ONEPASS);
    GemvT<double> gB, gBt;                       // t = B' w (p outputs) ; w = B vec (n outputs, via the stored transpose)
    gB.init(B.get(), d.ldx, n, p);
    if (!onepass) gBt.init(Bt.get(), ldbt, p, n);
    else Bt.release();
    { const bool nt = gemv_stream_nt(gB.bytes() + (onepass ? 0 : gBt.bytes())); gB.set_nt(nt); if (!onepass) gBt.set_nt(nt); }
    gB.run(w0.get(), AAAb.get(), nullptr, st);
    ADMM_HIP_CHECK(hipStreamSynchronize(st));
    S.t_factor = now_s() - t0;

    DenseLoop L;
    L.init(p, 1, opts, AAAb.get(), 0.0, st, res.trace_cap, res.state_cap);
    L.q.gout = gB.part.get(); L.q.gout_nseg = gB.pl.nseg; L.q.gout_stride = gB.stride;

    DevBuf<double> nvec, gpart;                  // one-pass form: B z (2), B y (2), B adj_y, w ; partial rows of the gather
    GatherPlan gp;
    GatherArgs<double> ga{};
    if (onepass) {
        const long long ldw = round_up(n, 32);
        nvec.alloc((size_t)6 * ldw); nvec.zero(st);
        gp = plan_gather<double>(n, p);
        gpart.alloc((size_t)gp.ngroups * gp.pstride); gpart.zero(st);
        ga = gather_args<double>(gp, B.get(), d.ldx, n, p, nullptr, gpart.get(), nullptr);
        L.q.bpn = n; L.q.w0 = w0.get();
        L.q.Bz0 = nvec.get(); L.q.Bz1 = nvec.get() + ldw; L.q.By0 = nvec.get() + 2 * ldw; L.q.By1 = nvec.get() + 3 * ldw;
        L.q.Badjy = nvec.get() + 4 * ldw; L.q.w = nvec.get() + 5 * ldw;
        L.q.gpart = gpart.get(); L.q.gngroups = gp.ngroups; L.q.gpstride = gp.pstride;
    }

    const int* skip = L.done.get();
    LoopTimes lt = run_until_done(st, skip, batch_iters((int)opt_int(Opt::BATCH_ITERS, 0), 8), (long long)opts.maxit + 2, [&](long long g) {
        L.head(g, st);
        if (onepass) {
            gB.run_partials(L.q.w, skip, st);               // B' w, w = B vec from the recurrences   (mat_vec_tprod, ADMMBP.h:66)
            L.tail(g, st);
            hipLaunchKernelGGL(bp_gather_kernel, dim3(gp.tiles, gp.ngroups), dim3(kGatherThreads), 0, st, L.q, (int)(g & 1), ga);      // B z_new
            return;
        }
        gBt.run_partials(L.vec.get(), skip, st);        // workspace = B vec   (mat_vec_prod,  ADMMBP.h:65)
        gB.run_partials_from(gBt, skip, st);            // B' workspace        (mat_vec_tprod, ADMMBP.h:66)
        L.tail(g, st);
    });
    S.t_loop = lt.wall_s; S.loop_ms_events = lt.events_ms; S.xupdate_launches = lt.launched;

    const DenseCtl fc = L.final_ctl(st);
    res.niter = fc.niter;
    S.total_iter = fc.niter; S.rho = fc.rho;
    dense_collect_trace(L, fc, res, st);
    const double* zfin = (fc.total & 1) ? L.z1.get() : L.z0.get();      // get_z() (BP.cpp:40)
    res.beta.assign(p, 0.0);
    read_back(res.beta.data(), zfin, (size_t)p * sizeof(double), st);
}

}  // namespace admm
