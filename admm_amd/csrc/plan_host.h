// Host scaffold of the lambda-path solvers (lasso_tall / lasso_wide / padmm_lasso / dantzig) and the dense loops: what each of them
// does around its own kernels, once -- the lambda grid, the read-out of a finished path, the control block after the loop, the form
// of the PEER exchange.  (The trace / iterate-dump recorders are LassoPlan's, solvers.h; the loop itself is loop_driver.h.)
#pragma once
#include "solvers.h"
#include "comm.h"
#include "box_host.h"
#include <climits>

namespace admm {

// The user grid (Lasso.cpp:78-89) into `user` and the internal grid lambda * n / scaleY (Lasso.cpp:99) into `internal`; returns
// nlambda.  `Round` is the type the internal value is rounded through before it is stored, and each solver keeps its own on
// purpose: float in the wide solver, double-of-float in the tall one (the reference's `Scalar lambda`), double in the consensus
// master (`double lambda`) and the Dantzig selector.
template <typename Round, typename Stored>
int make_path_grid(const LassoProblem& pb, double lambda0, long long n, double scaleY, std::vector<double>& user, std::vector<Stored>& internal) {
    user = make_lambda_grid(pb, lambda0, (int)n, scaleY);
    internal.resize(user.size());
    for (size_t i = 0; i < user.size(); ++i) internal[i] = (Stored)(Round)(user[i] * (double)n / scaleY);
    return (int)user.size();
}

// The common tail of a path: the iteration counts from the device, and the coefficient matrix on the original scale (DataStd::recover,
// Lasso.cpp:108-111) from the host snapshots `snap` (nlam x d.p) -- column l of `beta` is `stride` long, row 0 the intercept, this
// solver's columns from row 1 + col_offset.  Returns the sum of the counts, each clipped to `niter_clip`.  snap_stride: distance between the
// snapshots of two lambdas (0: d.p; the multi-task plan keeps m of them per lambda and reads them out response by response, each with
// its own mean `mean_y`; NULL: d.meanY).  box (admm_hip_boxenet; box_host.h): the recovered coefficients are clamped to the caller's
// bounds, and where the clamp moved one the intercept is taken again from the clamped coefficients (recover_coef's sum, in its order);
// a path that the clamp leaves alone -- every path without bounds -- keeps recover_coef's bits.
template <typename T>
long long read_out_path(const DeviceData<T>& d, const T* snap, int nlam, const int* dev_niter, size_t stride, long long col_offset,
                        std::vector<int>& niter, std::vector<T>& beta, int niter_clip = INT_MAX, size_t snap_stride = 0,
                        const T* mean_y = nullptr, const BoxClamp* box = nullptr) {
    if (snap_stride == 0) snap_stride = (size_t)d.p;
    niter.assign(nlam, 0);
    ADMM_HIP_CHECK(hipMemcpy(niter.data(), dev_niter, (size_t)nlam * sizeof(int), hipMemcpyDeviceToHost));
    beta.assign(stride * nlam, T(0));
    long long tot = 0;
    for (int l = 0; l < nlam; ++l) {
        T b0 = 0;
        T* out = beta.data() + (size_t)l * stride + 1 + col_offset;
        recover_coef<T>(d, mean_y ? *mean_y : d.meanY, snap + (size_t)l * snap_stride, &b0, out);
        if (box != nullptr && box->on() && box->apply(out, d.p) && (d.flag & 2)) {
            T acc = T(0);
            for (int j = 0; j < d.p; ++j) acc += out[j] * d.meanX[j];
            b0 = (mean_y ? *mean_y : d.meanY) - acc;
        }
        beta[(size_t)l * stride] = b0;
        tot += std::min(niter[l], niter_clip);
    }
    return tot;
}

// Both slots of a double-buffered control block once the loop has ended (the stream is idle).
template <typename Ctl>
struct CtlPair {
    Ctl c[2];
    long long total() const { return std::max(c[0].total, c[1].total); }      // decisions taken = the cold-start one + one per ADMM iteration
    const Ctl& finished() const { return c[0].done ? c[0] : c[1]; }
};
template <typename Ctl>
CtlPair<Ctl> read_ctl(const Ctl* dev) {
    CtlPair<Ctl> h;
    ADMM_HIP_CHECK(hipMemcpy(h.c, dev, sizeof(h.c), hipMemcpyDeviceToHost));
    return h;
}

// admm_stats.exchange_variant: 0 nothing travels, 1 the exchange layer's all-reduce, 2 the solver's own kernels over PEER slots,
// 3 ... producer and consumer in one launch.
inline int exchange_variant(bool sharded, bool fused, bool one) { return !sharded ? 0 : (!fused ? 1 : (one ? 3 : 2)); }

// How a sharded solver exchanges per iteration.  fused: by its own kernels over the PEER back-end (ADMM_HIP_PEER_FUSED=0: through the
// generic all-reduce of the exchange layer there too).  one: producer and consumer in ONE launch (`one_kernel`, `block` threads,
// `grid` workgroups) -- only when the whole grid is resident with room to spare, because its workgroups wait for one another
// (ADMM_HIP_PEER_FUSED=2: never).
struct ExchangeForm { bool fused = false, one = false; int variant = 0; };
inline ExchangeForm peer_exchange_form(bool sharded, const CommInfo& ci, const void* one_kernel, int block, long long grid) {
    ExchangeForm f;
    f.fused = sharded && ci.backend == COMM_PEER && !opt_is(Opt::PEER_FUSED, "0");
    if (f.fused) {
        int occ = 0;
        ADMM_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, one_kernel, block, 0));
        f.one = grid * 2 <= resident_workgroups(occ) && !opt_is(Opt::PEER_FUSED, "2");
    }
    f.variant = exchange_variant(sharded, f.fused, f.one);
    return f;
}

}  // namespace admm
