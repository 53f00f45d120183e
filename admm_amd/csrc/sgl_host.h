// Host side of the sparse-group lasso (admm_hip_sgl): the three weights the device sees and lambda_0 of the automatic grid.  Plain
// C++, no HIP: included by call_args.h / lasso_tall.hip and reachable without a device through admm_hip_host_sgl_lambda0.
//
// Penalty, in the solver's internal units:  lambda [ alpha sum_j u_j |b_j| + (1 - alpha) sum_g w_g ||b_g||_2 ].
// The device never sees alpha.  It gets, in double,
//     l1_j = alpha u_j                     the element-wise threshold weight inside a group of several columns,
//     wg_g = (1 - alpha) w_g               the block threshold weight of such a group,
//     ws_j = l1_j + wg_g                   the one threshold weight of a group of ONE column (|b| is both norms there),
// and forms every threshold as lambda * weight / rho.  alpha = 0 gives l1 = 0, wg = w exactly (the group lasso); alpha = 1 gives
// l1 = u, wg = 0 exactly (the Lasso with penalty factors u).
#pragma once
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

namespace admm {

// l1[p] and wg[ngroups] from the caller's u (NULL: all 1) and w (NULL: sqrt(group size)); group g = columns [start[g], start[g + 1])
inline void sgl_prepare(double alpha, const double* u, const double* w, const std::vector<int>& start,
                        std::vector<double>& l1, std::vector<double>& wg) {
    const int ng = (int)start.size() - 1, p = start.back();
    const double beta = 1.0 - alpha;
    l1.resize(p); wg.resize(ng);
    for (int j = 0; j < p; ++j) l1[j] = alpha * (u ? u[j] : 1.0);
    for (int g = 0; g < ng; ++g) wg[g] = beta * (w ? w[g] : std::sqrt((double)(start[g + 1] - start[g])));
}

// The weight of a one-column group: the two prepared weights added (each already rounded, so no contraction can change the sum).
inline double sgl_single_weight(double l1_j, double wg_g) { return l1_j + wg_g; }

// lambda_g of one group: the smallest lambda at which the prox of the whole penalty empties the group started from c = X'y, i.e. the
// root of  f(lambda) = sum_j max(|c_j| - lambda a_j, 0)^2 - (b lambda)^2  (a = l1 of the group's columns, b = wg; f is piecewise
// quadratic and non-increasing).  Solved exactly: the piece that holds the sign change is found over the sorted breakpoints
// |c_j| / a_j, and on it  f = A l^2 - 2 B l + C  with the sums over the columns still above their threshold, taken in column order.
// Returns a negative value for a group that no lambda empties (b = 0 and a column with a_j = 0, c_j != 0).
inline double sgl_group_lambda(const float* c, const double* a, int gn, double b) {
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> t;                       // finite breakpoints of the columns that matter
    bool never = false;                          // a column with c != 0 that the l1 part cannot remove
    for (int j = 0; j < gn; ++j) {
        const double cj = std::fabs((double)c[j]);
        if (cj == 0.0) continue;
        if (a[j] > 0) t.push_back(cj / a[j]); else never = true;
    }
    if (t.empty() && !never) return 0.0;         // c_g = 0: empty at every lambda
    if (!(b > 0)) {
        if (never) return -1.0;
        return *std::max_element(t.begin(), t.end());      // no block part: the last column leaves at its own breakpoint
    }
    std::sort(t.begin(), t.end());
    const auto tj = [&](int j) { const double cj = std::fabs((double)c[j]); return cj == 0.0 ? 0.0 : (a[j] > 0 ? cj / a[j] : inf); };
    const auto f = [&](double lam) {
        double s = 0.0;
        for (int j = 0; j < gn; ++j) { const double r = std::fabs((double)c[j]) - lam * a[j]; if (r > 0) s += r * r; }
        const double bl = b * lam;
        return s - bl * bl;
    };
    // the first breakpoint at which f <= 0 (f is monotone): the root lies in (lo, hi], where the active columns are those with t_j > lo
    size_t k0 = 0, k1 = t.size();
    while (k0 < k1) { const size_t m = (k0 + k1) / 2; if (f(t[m]) <= 0) k1 = m; else k0 = m + 1; }
    const double lo = k0 > 0 ? t[k0 - 1] : 0.0, hi = k0 < t.size() ? t[k0] : inf;
    double A = -(b * b), B = 0.0, C = 0.0;
    for (int j = 0; j < gn; ++j) {
        if (!(tj(j) > lo)) continue;
        const double cj = std::fabs((double)c[j]);
        A += a[j] * a[j]; B += a[j] * cj; C += cj * cj;
    }
    double lam;
    if (B == 0.0) lam = std::sqrt(C) / b;        // no l1 weight on what is left: the group lasso's rule ||c_g|| / w_g, to the bit
    else {
        const double D = B * B - A * C;
        lam = C / (B + std::sqrt(D > 0 ? D : 0.0));           // the root on the falling branch, in the form without cancellation
    }
    return std::min(std::max(lam, lo), hi);
}

// lambda_0 = max_g lambda_g over the groups that some lambda empties, rounded to float like the Lasso's `Scalar lambda0`.
inline float sgl_lambda0(const float* xy, const std::vector<int>& start, const std::vector<double>& l1, const std::vector<double>& wg) {
    double best = 0.0;
    for (size_t g = 0; g + 1 < start.size(); ++g)
        best = std::max(best, sgl_group_lambda(xy + start[g], l1.data() + start[g], start[g + 1] - start[g], wg[g]));
    return (float)best;
}

}  // namespace admm
