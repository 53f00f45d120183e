// Host side of the box-constrained, weighted elastic net (admm_hip_boxenet): the bounds in the solver's units, lambda_0 of the automatic
// grid and the clamp of the recovered coefficients.  Plain C++, no HIP: included by call_args.h / plan_host.h / lasso_tall.hip and
// reachable without a device through admm_hip_host_box_lambda0.
//
// Problem, in the solver's internal units:
//     minimise 1/2 ||y_s - X_s b||^2 + lambda sum_j u_j [ alpha |b_j| + (1 - alpha)/2 b_j^2 ]   subject to   lo_j <= b_j <= hi_j ,
// with lo_j <= 0 <= hi_j.  The caller gives the bounds on the ORIGINAL coefficient scale (beta_j = b_j scaleY / scaleX_j), so
//     lo_j (solver) = lower_j scaleX_j / scaleY ,
// formed in double and rounded to float TOWARDS THE INSIDE of the box: a z the device clamps to such a bound is never outside the
// caller's interval by more than the float rounding of the recovery, which the clamp of the output (below) removes.
#pragma once
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

namespace admm {

// The float nearest to v inside the box: not below v for a lower bound, not above v for an upper one.  Infinite bounds stay infinite;
// a finite bound beyond the float range becomes -+FLT_MAX; the sign of a zero is dropped (0 is +0).
inline float box_round_lower(double v) {
    float f = (float)v;
    if ((double)f < v) f = std::nextafterf(f, std::numeric_limits<float>::infinity());
    return f + 0.0f;
}
inline float box_round_upper(double v) {
    float f = (float)v;
    if ((double)f > v) f = std::nextafterf(f, -std::numeric_limits<float>::infinity());
    return f + 0.0f;
}

// One bound into the solver's units (scale_x, scale_y: the standardisation's; both 1 where that part is off).  An infinite bound needs
// no product (and a constant column's scale must not turn it into NaN).
inline double box_to_std(double bound, double scale_x, double scale_y) {
    return std::isinf(bound) ? bound : bound * scale_x / scale_y;
}

// lambda_0 of the automatic grid from c = X_s'y_s: the smallest lambda at which the prox started from c leaves every penalised
// coordinate at zero.  Coordinate j leaves zero upwards only if it may (hi_j > 0) and c_j > lambda u_j, downwards only if lo_j < 0 and
// -c_j > lambda u_j:   lambda_0 = max over u_j > 0 of g_j / u_j ,  g_j = max(c_j if hi_j > 0 else 0, -c_j if lo_j < 0 else 0),
// in double from the float c, rounded to float like the Lasso's `Scalar lambda0`.  lo, hi NULL: no bounds; u NULL: all 1 -- then the
// value is max |c_j| to the bit (device_absmax).  The elastic net divides by alpha + 1e-4 afterwards, as ADMMEnet.h:56 (box_lambda0_enet).
inline float box_lambda0(const float* c, int p, const float* lo, const float* hi, const double* u) {
    double best = 0.0;
    for (int j = 0; j < p; ++j) {
        const double uj = u ? u[j] : 1.0;
        if (!(uj > 0)) continue;
        const double cj = (double)c[j];
        const double up = (!hi || hi[j] > 0.f) ? cj : 0.0, down = (!lo || lo[j] < 0.f) ? -cj : 0.0;
        best = std::max(best, std::max(up, down) / uj);
    }
    return (float)best;
}
inline float box_lambda0_enet(float lambda0, double alpha) { return (float)(lambda0 / ((double)(float)alpha + 0.0001)); }

// The caller's box rounded inwards to float, for the clamp of the recovered coefficients: lower_j <= beta_j <= upper_j then holds
// exactly in the output (compared in double).  Empty vectors: no bounds.
struct BoxClamp {
    std::vector<float> lo, hi;
    bool on() const { return !lo.empty(); }
    void set(const std::vector<double>& lower, const std::vector<double>& upper) {
        lo.resize(lower.size()); hi.resize(upper.size());
        for (size_t j = 0; j < lower.size(); ++j) { lo[j] = box_round_lower(lower[j]); hi[j] = box_round_upper(upper[j]); }
    }
    // Clamp p recovered coefficients in place; returns whether any of them moved (with infinite bounds none can).
    template <typename T>
    bool apply(T* beta, int p) const {
        bool moved = false;
        for (int j = 0; j < p; ++j) {
            if (beta[j] < (T)lo[j]) { beta[j] = (T)lo[j]; moved = true; }
            else if (beta[j] > (T)hi[j]) { beta[j] = (T)hi[j]; moved = true; }
        }
        return moved;
    }
};

}  // namespace admm
