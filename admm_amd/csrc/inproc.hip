// In-process ranks of a PAR_DEVICES call (inproc.h).
#include "inproc.h"
#include "comm.h"
#include <algorithm>
#include <condition_variable>
#include <mutex>
#include <thread>

namespace admm {

std::vector<int> par_layout(int nblocks, const std::vector<int>& listed) {
    int nr = 1;
    for (int d = std::min<int>((int)listed.size(), nblocks); d >= 1; --d) if (nblocks % d == 0) { nr = d; break; }
    return nr > 1 ? std::vector<int>(listed.begin(), listed.begin() + nr) : std::vector<int>();
}
static thread_local std::vector<int> t_last_layout;
const std::vector<int>& last_layout() { return t_last_layout; }
void record_single_layout() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = 0; }
    t_last_layout.assign(1, dev);
}

// One persistent host thread per rank index, re-used by every in-process call of the process: a rank's thread keeps its pooled
// streams, pinned staging ring and BLAS handle from one call to the next (creating them costs more than a small solve), and nothing
// is left behind per call.  Never destroyed (the runtime may be gone at process exit).
namespace {
struct RankWorker {
    std::mutex mu;
    std::condition_variable cv;
    std::function<void()> task;
    bool busy = false;
    RankWorker() { std::thread([this] { loop(); }).detach(); }
    void loop() {
        for (;;) {
            std::function<void()> t;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return (bool)task; });
                t = std::move(task);
                task = nullptr;
            }
            t();
            { std::lock_guard<std::mutex> lk(mu); busy = false; }
            cv.notify_all();
        }
    }
    void start(std::function<void()> f) {
        { std::lock_guard<std::mutex> lk(mu); task = std::move(f); busy = true; }
        cv.notify_all();
    }
    void wait() {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return !busy; });
    }
};
std::mutex& inproc_mu() { static std::mutex* m = new std::mutex(); return *m; }     // one in-process call at a time per process
RankWorker& rank_worker(int r) {
    static std::vector<RankWorker*>* w = new std::vector<RankWorker*>();
    while ((int)w->size() <= r) w->push_back(new RankWorker());
    return *(*w)[r];
}

struct RankOutcome { int code = ADMM_OK; std::string msg; bool abandoned = false; std::vector<DeferredFree> frees; };
}  // namespace

void run_inproc(const std::vector<int>& devices, int src_device, const std::function<void(int, int)>& body) {
    ADMM_REQUIRE(!comm_process_attached(), "PAR_DEVICES (in-process ranks) cannot be combined with an attached process-wide communicator "
                                           "(admm_hip_comm_init*): use the *_dist entry points there, or finalize it first");
    std::lock_guard<std::mutex> call_lock(inproc_mu());
    const int nranks = (int)devices.size();
    int cur = 0;
    ADMM_HIP_CHECK(hipGetDevice(&cur));
    if (src_device >= 0) {
        for (int d : devices) {
            if (d == src_device) continue;
            int can = 0;
            ADMM_HIP_CHECK(hipDeviceCanAccessPeer(&can, d, src_device));
            ADMM_REQUIRE(can, "PAR_DEVICES with device input: device " + std::to_string(d) + " cannot read device " + std::to_string(src_device) +
                              "'s memory (no peer access); pass the input in host memory instead");
            ADMM_HIP_CHECK(hipSetDevice(d));
            const hipError_t pe = hipDeviceEnablePeerAccess(src_device, 0);
            (void)hipSetDevice(cur);
            if (pe == hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
            else ADMM_HIP_CHECK(pe);
        }
    }
    std::vector<int> sorted(devices);
    std::sort(sorted.begin(), sorted.end());
    const bool shared = std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end();
    const ThreadOptions opts = thread_options();
    InprocGroup* g = comm_group_create(devices);
    std::vector<RankOutcome> out(nranks);
    for (int r = 0; r < nranks; ++r) {
        rank_worker(r).start([&, r]() {
            thread_options() = opts;
            if (shared) { opt_set_thread(Opt::PEER_FUSED, "2"); opt_set_thread(Opt::PAR_FUSE_PZ, "0"); }
            RankOutcome& o = out[r];
            defer_frees(&o.frees);
            try {
                ADMM_HIP_CHECK(hipSetDevice(devices[r]));
                comm_group_attach(g, r);
                if (opt_int(Opt::TEST_PAR_FAIL_RANK, -1) == r)           // test hook: this rank fails on the host before its first exchange
                    throw Error(ADMM_ERR_INTERNAL, "test: injected failure of rank " + std::to_string(r));
                body(r, nranks);
            } catch (const Error& e) {
                o.code = e.code; o.msg = e.what();
            } catch (const std::bad_alloc&) {
                o.code = ADMM_ERR_INTERNAL; o.msg = "host allocation failed";
            } catch (const std::exception& e) {
                o.code = ADMM_ERR_INTERNAL; o.msg = e.what();
            }
            if (o.code != ADMM_OK) {
                o.abandoned = o.code == ADMM_ERR_COMM && o.msg.rfind("exchange abandoned", 0) == 0;
                o.msg = "rank " + std::to_string(r) + " (device " + std::to_string(devices[r]) + "): " + o.msg;
                comm_group_abort(g);
            }
            comm_group_detach();
            defer_frees(nullptr);
            thread_options() = ThreadOptions();
        });
    }
    for (int r = 0; r < nranks; ++r) rank_worker(r).wait();
    for (int r = 0; r < nranks; ++r) {                  // every rank has returned: its releases are safe now
        (void)hipSetDevice(devices[r]);
        release_deferred(out[r].frees);
    }
    comm_group_destroy(g);
    (void)hipSetDevice(cur);
    t_last_layout = devices;
    int first = -1;
    for (int r = 0; r < nranks && first < 0; ++r) if (out[r].code != ADMM_OK && !out[r].abandoned) first = r;
    for (int r = 0; r < nranks && first < 0; ++r) if (out[r].code != ADMM_OK) first = r;
    if (first >= 0) throw Error(out[first].code, out[first].msg);
}

std::vector<int> par_devices_for(int nblocks) {
    return par_layout(nblocks, parse_par_devices(opt_text(Opt::PAR_DEVICES), admm_hip_device_count()));
}
int input_device(const void* x, int mem) {
    if (mem != ADMM_MEM_DEVICE) return -1;
    hipPointerAttribute_t at;
    ADMM_HIP_CHECK(hipPointerGetAttributes(&at, x));
    return at.device;
}

}  // namespace admm
