// Every named option of the library -- variant selectors, tuning and test values -- declared once (INTEGRATION.md §5 documents the
// same names).  A value is checked and parsed when it is set (admm_hip_option_set, admm_hip_options_set, the ADMM_HIP_<NAME>
// environment overlay); call sites read the typed value by identifier: opt_off(Opt::WIDE_FUSE).
#pragma once
#include <limits>
#include <string>
#include <vector>

namespace admm {

enum class OptKind { Flag, Int, Real, Choice, Text, Sched, Devices };
struct OptAccepts {
    OptKind kind;
    double lo = 0, hi = 0;            // Int / Real: the inclusive range
    const char* choices = nullptr;    // Choice: "a|b|c"
};
constexpr OptAccepts Flag() { return {OptKind::Flag, 0, 1}; }
constexpr OptAccepts Int(double lo, double hi) { return {OptKind::Int, lo, hi}; }
constexpr OptAccepts Real(double lo, double hi) { return {OptKind::Real, lo, hi}; }
constexpr OptAccepts Choice(const char* c) { return {OptKind::Choice, 0, 0, c}; }
constexpr OptAccepts Text() { return {OptKind::Text}; }
constexpr OptAccepts Sched() { return {OptKind::Sched}; }          // "big,small,split‰": widths 32 .. 256 in steps of 32, split 0 .. 1000
constexpr OptAccepts Devices() { return {OptKind::Devices}; }      // "0", "all" or a comma-separated list of device numbers
constexpr double kPositive = std::numeric_limits<double>::min();  // Real(kPositive, ...): any value > 0

// X(identifier / name, accepted values, summary)
#define ADMM_OPTIONS(X)                                                                                                                  \
    X(BATCH_ITERS, Int(1, 1 << 20), "iterations enqueued between two host polls (rounded up to even; default per solver)")             \
    X(PROFILE_STRIDE, Int(0, 1 << 30), "time every k-th tall x-update launch with HIP events (0: off)")                                 \
    X(GRAM, Choice("rocblas|oneshot"), "tall Gram through rocBLAS / host input transferred before the Gram is built")                    \
    X(GRAM_SPLIT, Choice("0|f16x2|bf16x3"), "tall Gram of order >= ~4000: exact fp32 kernel / fp16 x 2 (default) / bf16 x 3")          \
    X(GRAM_B3_KTILES, Int(0, 1 << 20), "K tiles per launch of the 16-bit split Gram (0: one launch)")                                   \
    X(FACTOR, Choice("rocsolver"), "Cholesky + inverse through rocSOLVER / rocBLAS instead of the hand-written kernels")                \
    X(INVERSE, Choice("f32|f64"), "precision the cached inverse is built in")                                                           \
    X(XUPDATE, Choice("sym|gemv|full"), "tall x-update: symmetric lower-triangle kernel / full-matrix mat-vec (gemv and full alike)")   \
    X(SYMV_SCHED, Sched(), "tall x-update: column-segment widths of the long / short row strips and the split between them")           \
    X(SYMV_VERDICT, Choice("0|1|2|3"), "tall x-update: discarded launches stream on / leave on block 0's word at start / also mid-tile / every tile decides first, one vector (default)") \
    X(SYMV_PACK, Choice("0|1"), "tall x-update, decide-first form: stream the fp32 inverse / its exact 29-bit copy (default)")          \
    X(SYMV_PACK_ESC, Int(0, 4096), "tall x-update: entries a tile of the 29-bit copy may hold outside its exponent window (default 32; one tile beyond it: the fp32 stream)") \
    X(REFINE, Flag(), "tall path: refine every x-update with a double-precision residual")                                               \
    X(DIST_FACTOR, Flag(), "row-sharded tall solver: 0 = every rank factorises the whole all-reduced Gram")                            \
    X(CV_DOWNDATE, Flag(), "cross-validation folds' Grams as down-dates of the full-data Gram: 1 always, 0 never")                      \
    X(PREP_FUSED, Flag(), "0: convert, column statistics and standardisation as separate sweeps over X")                                \
    X(H2D, Choice("pageable"), "host inputs through plain hipMemcpy instead of the pinned staging ring")                                 \
    X(POOL_MB, Int(0, 1 << 30), "cache of released device blocks, megabytes (0: off)")                                                  \
    X(WIDE_FUSE, Flag(), "wide path: 0 = three launches per iteration")                                                                  \
    X(WIDE_TGLOBAL, Flag(), "wide path: 1 = t through global memory instead of LDS")                                                     \
    X(WIDE_SPRAD, Choice("gram"), "wide path: spectral radius from the explicit n x n Gram")                                            \
    X(WIDE_SCREEN, Choice("0|8|16|auto"), "wide path: screen the regular steps never / 8-bit code / fp16 copy / chosen at any size")    \
    X(WIDE_SCREEN_STATS, Flag(), "wide path: print the screen's counts")                                                                 \
    X(WIDE_PERSIST, Flag(), "wide path: 0 = no persistent active-set stretches")                                                         \
    X(WIDE_PERSIST_COLS, Flag(), "column-sharded wide solver: 0 = no persistent active-set stretches")                                  \
    X(WIDE_ROWS_C, Int(1, 32), "wide path: column groups of the 2-D stretch (kept only when it fits with the problem's row groups)")    \
    X(WIDE_PERSIST_STATS, Flag(), "wide path: print the stretch statistics")                                                             \
    X(PAR_ONEPASS, Flag(), "consensus solver: 0 = the reference's two products per Woodbury worker")                                    \
    X(PAR_ONEPASS_TAU, Real(0, 1e300), "one-pass Woodbury workers: threshold of the cancellation guard (0: never fall back)")           \
    X(PAR_ONEPASS_STATS, Flag(), "one-pass Woodbury workers: print how many worker-iterations took the dense pass")                     \
    X(PAR_FUSE_PZ, Flag(), "consensus solver: 0 = pack and z as two launches")                                                           \
    X(PAR_BATCH, Flag(), "consensus solver: 0 = one launch per worker and product")                                                      \
    X(PAR_DEVICES, Devices(), "admm_hip_parlasso / admm_hip_parbp over several devices in one process")                                \
    X(TEST_PAR_FAIL_RANK, Int(0, 63), "test hook: this rank of an in-process call fails before its first exchange")                    \
    X(PEER_FUSED, Choice("0|1|2"), "PEER back-end: 0 = the generic all-reduce, 2 = producer and consumer as two launches")             \
    X(PEER_MEM, Choice("uncached"), "PEER exchange buffers as uncached device memory")                                                   \
    X(COMM_SLOT_BYTES, Int(4096, 1ll << 40), "payload capacity of one PEER / SHM exchange (rounded down to 16 bytes)")                 \
    X(COMM_TIMEOUT_S, Real(kPositive, 1e300), "wait bound of the per-iteration exchanges, seconds")                                    \
    X(COMM_PATIENT_TIMEOUT_S, Real(kPositive, 1e300), "wait bound of setup reductions and replica joins, seconds")                     \
    X(LAD_HAT, Flag(), "LAD: 0 = the general projection also for n <= 2000")                                                            \
    X(LAD_ONEPASS, Flag(), "LAD: 0 = the reference's two products per iteration")                                                      \
    X(QUANT_SLOTS, Int(0, 8), "admm_hip_quantreg, admm_hip_huber: fits per pass over X on the one-pass branch: 0 = automatic, 1 = serial, else at most that many") \
    X(MT_RHS, Choice("0|2|4|8|12"), "admm_hip_mtlasso: right-hand sides per pass over the cached inverse (0: automatic)")               \
    X(BP_ONEPASS, Flag(), "basis pursuit: 0 = the reference's two products per iteration")                                             \
    X(SBP_GRAM, Flag(), "admm_hip_parbp: 0 = the direct launches on every active-set iteration")                                       \
    X(SBP_GRAM_CAP, Int(1, 1024), "admm_hip_parbp: most columns of the Gram-space matrix (rounded to multiples of 8)")                 \
    X(SBP_GRAM_CARRY, Flag(), "admm_hip_parbp: 0 = every Gram-space stretch starts from the direct launches' n-vectors")              \
    X(SBP_SCREEN, Flag(), "admm_hip_parbp: screen the regular iterations always / never")                                             \
    X(SBP_SCREEN_STATS, Flag(), "admm_hip_parbp: print the screen's counts")                                                           \
    X(SBP_WGS, Int(1, 1 << 20), "admm_hip_parbp: workgroups of the x-update launches")                                                 \
    X(SBP_SHARE, Int(1, 1 << 20), "admm_hip_parbp: smallest share of a block's non-zero list a workgroup takes")                      \
    X(SBP_TEST_DELAY_US, Int(0, 1000000), "test hook: every even workgroup of a Gram-space launch starts that many us late")           \
    X(TEST_RESIDENT_WGS, Int(0, 1ll << 40), "test hook: pretend the device holds that many resident workgroups")                      \
    X(TEST_FREE_BYTES, Int(0, 1ll << 52), "test hook: pretend the device has that many bytes free")                                    \
    X(PROBE_OUT, Text(), "dev build with in-kernel timestamps (-DADMM_HIP_PROBE): file the probe records go to")

enum class Opt : int {
#define ADMM_OPT_ID(id, accepts, summary) id,
    ADMM_OPTIONS(ADMM_OPT_ID)
#undef ADMM_OPT_ID
};
constexpr int kNumOptions = 0
#define ADMM_OPT_COUNT(id, accepts, summary) +1
    ADMM_OPTIONS(ADMM_OPT_COUNT)
#undef ADMM_OPT_COUNT
    ;

// A value as it was set (text) and parsed: Flag / Int -> i, Real -> r, Choice -> i = its place in the list, Sched -> sched.
struct OptValue {
    std::string text;
    long long i = 0;
    double r = 0;
    int sched[3] = {0, 0, 0};
};
// The options of one thread: what it set through the C ABI; unset entries fall through to the environment overlay.
struct ThreadOptions {
    bool has[kNumOptions] = {};
    OptValue v[kNumOptions];
};

// The value in force for the CALLING THREAD -- its own setting, else the process-wide overlay of the ADMM_HIP_<NAME> environment
// variables captured once when the library is first used -- or nullptr for "library default".  Valid until the thread changes
// its options.
const OptValue* opt(Opt id);
inline bool opt_set(Opt id) { return opt(id) != nullptr; }
inline long long opt_int(Opt id, long long dflt) { const OptValue* v = opt(id); return v ? v->i : dflt; }      // Flag, Int
inline double opt_real(Opt id, double dflt) { const OptValue* v = opt(id); return v ? v->r : dflt; }
inline const char* opt_text(Opt id) { const OptValue* v = opt(id); return v ? v->text.c_str() : nullptr; }
inline bool opt_on(Opt id) { return opt_int(id, -1) == 1; }        // a flag set to 1
inline bool opt_off(Opt id) { return opt_int(id, -1) == 0; }       // a flag set to 0
bool opt_is(Opt id, const char* choice);                           // a choice option set to this value of its list

// Iterations per host poll: BATCH_ITERS (captured as `set`, 0 = unset) rounded up to even, or the solver's own default.
inline int batch_iters(int set, int dflt) { return set > 0 ? (set + 1) / 2 * 2 : dflt; }

// The C ABI's side (api.hip) and the in-process ranks' copy of the caller's settings.  Names are case-insensitive, the ADMM_HIP_ prefix optional; an unknown name or a value outside what
// the option accepts throws ADMM_ERR_INVALID_ARG and changes nothing.
bool opt_find(const char* name, Opt* id);
void opt_parse(Opt id, const char* text, OptValue* out);
ThreadOptions& thread_options();
void opt_set_thread(Opt id, const char* value);                   // value nullptr: back to the default / overlay
void check_option_overlay();                                       // throws when an ADMM_HIP_<NAME> variable holds a malformed value
// PAR_DEVICES: "0" / "" / unset: off (empty list).  "all": devices 0 .. device_count - 1.  Else the listed device numbers (repeats
// allowed: several ranks on one device -- the test / diagnostic form).
std::vector<int> parse_par_devices(const char* v, int device_count);

}  // namespace admm
