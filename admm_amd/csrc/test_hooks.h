// The test hooks behind the C ABI (include/admm_hip.h, "test hooks"): test_hooks.hip, and cv.hip for the fold system.
#pragma once

namespace admm {

void test_symv(const float* A, int p, const float* v0, const float* v1, float* y0, float* y1);
void test_symv_multi(const float* A, int p, const float* V, int nr, int rhs_per_pass, float* Yout);
constexpr int kSymvHookMaxP = 32768;      // largest order the hooks below accept
bool test_symv_rhs_built(int rhs_per_pass);      // one of the widths symvn_lower_kernel is built for (kSyNR, symv_kernels.h)
void test_symv_plan(int p, int cus, int part, int nparts, int* sched_out, long long* info_out, int* tiles_out, int tile_capacity);      // host only
void test_symv_ex(const float* A, int p, const float* v0, const float* v1, int variant, int part, int nparts, float* y0, float* y1, int* sched_out);
void test_symv_one(const float* A, int p, const float* v0, const float* v1, int gate, int nt, unsigned fill, float* y, float* dot_out, float* axp_out,
                   long long plane_capacity, long long* info_out, int* sched_out);
void test_symv_pack_host(const unsigned* bits, int nchunks, int* base_io, unsigned* stream_out, unsigned* esc_out, int esc_cap, long long* nesc_out,
                         unsigned* decoded_out);      // host only
void test_symv_packed(const float* A, int p, const float* v0, const float* v1, int gate, int nt, unsigned fill, int esc_cap, float* y, float* dot_out,
                      float* axp_out, long long plane_capacity, long long* info_out, int* sched_out);
void test_symv_packed_time(const float* A, int p, const float* v0, int reps, float* us_out, long long* info_out);
void test_symv_multi_ex(const float* A, int p, const float* V, int nr, int rhs_per_pass, int nt, int finish, float* Yout, int* sched_out);
void test_symv_f64acc(const float* A, int p, const float* v0, const float* v1, double* y0, double* y1, int* sched_out);
template <typename T> void test_gram(const T* A, int rows, int cols, bool atA, T* G);
template <typename T> void test_spd_inverse(const T* A, int n, T* Ainv, bool via64);
void test_spd_inverse_shift(const float* A, int n, double diag, float* Ainv);
template <typename T> void test_cholesky_linvt(const T* A, int n, T* L, T* U);
template <typename T> void test_gemm_nt(bool lower, bool mirror, bool kstart_row, bool b_lower, bool in_place, int M, int N, int K, double alpha, double beta,
                                        const T* A, const T* B, T* C);
template <typename T> void test_gemv_t(const T* A, int rows, int cols, const T* v, T* y);
constexpr int kGemvHookMaxCount = 8;      // products of one admm_hip_test_gemv_t_ex call
struct GemvExRequest {                    // admm_hip_test_gemv_t_ex's arguments, checked by api.hip as far as that goes without a device
    int form, nrhs, nt, max_seg_rows, lda_extra, count;
    unsigned long long fill;
    const int* m; const int* k; const void* const* A; const void* const* v; const int* from; const int* skip;
    void* const* part_out; long long part_capacity; void* const* y_out; long long* info_out;
};
template <typename T> void test_gemv_t_ex(const GemvExRequest& q);
void test_wide_op(const float* X, int n, int p, const float* v, float* w);
void test_block_sprad(const double* A, int n, int p, int nblocks, double* out, int* nsteps_out);      // sharing_bp.hip
double block_sprad_bytes(int n, int nblocks);      // sharing_bp.hip: device bytes of one batch of nblocks Lanczos runs (host only)
struct WideScreenLayout { long long ldh; int S; };      // lasso_wide.hip: leading dimension of the screen's copy, stride of its [NW][S] bound / scale arrays
WideScreenLayout wide_screen_layout(int n, int p, int fmt, int NW);      // (host only) what WidePlan::setup_screen and the hook below both use
void test_wide_screen_prep(const float* X, int n, int p, int fmt, int nw, unsigned pad_fill, void* copy_out, float* s_out, float* scale_out,
                           double* rate_out, long long* info_out);      // lasso_wide.hip
long long sbp_screen_ldh(int n);      // sharing_bp.hip (host only)
void test_sbp_screen_prep(const double* A, int n, int pl, int lda_extra, unsigned pad_fill, unsigned short* copy_out, float* s_out,
                          long long* info_out);      // sharing_bp.hip
template <typename T> void test_gather(const T* A, int rows, int cols, const T* v, double* y);
void test_cv_fold_system(const double* x, const double* y, int n, int p, const int* fold_id, int nfolds, int fold,
                         int standardize, int intercept, float* gram, float* xy, float* mean_x, float* scale_x, float* mean_scale_y);
long long tall_last_early_exits();      // lasso_tall.hip
void tall_last_pack_info(long long* out);      // lasso_tall.hip
constexpr int kTallGateHookMaxNwg = 1 << 16;
void test_tall_gate(const double* ctl_d, const int* ctl_i, const double* compact, int nwg, int maxit, int nlam, double* sums_out,
                    int* answer_out);      // lasso_tall.hip (TallGate lives there): a tile's decision on caller-supplied inputs
void test_tall_norms(const double* rows, int nwg, double* sums_out);      // lasso_tall.hip: block 0's six sums from the rows of P
void test_logit_prox(const double* v, long long m, double t, double* out);      // fadmm_dense.hip: the device logit2 over a host array
void test_poisson_prox(const double* v, const double* y, long long m, double t, double* out);      // fadmm_dense.hip: the device pois2 over host arrays

}  // namespace admm
