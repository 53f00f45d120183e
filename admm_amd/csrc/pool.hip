// Cache of large device blocks behind DevBuf, and the deferred releases of in-process ranks (admm_internal.h).
#include "admm_internal.h"
#include <mutex>

namespace admm {

namespace {
struct PoolBlock { void* p; size_t bytes; int dev; };
struct Pool {
    std::mutex mu;
    std::vector<PoolBlock> blocks;
    size_t cached = 0;
};
Pool& pool() { static Pool* p = new Pool(); return *p; }             // never destroyed: the runtime may be gone at process exit
constexpr size_t kPoolMinBytes = size_t(32) << 20;
// Cap of the cache: ADMM_HIP_POOL_MB, default the smaller of 16 GB and an eighth of the device's memory (24 GB held back from
// every other allocator of the process -- library workspaces, RCCL, torch, an R session -- was too much to keep silently; what a warm
// C2 setup re-uses is ~10 GB).  Allocators of this library that bypass DevBuf (the PEER exchange buffer) trim the cache and retry on
// out-of-memory themselves; admm_hip_trim_memory() hands everything back on request.
size_t pool_cap_bytes() {
    if (opt_set(Opt::POOL_MB)) return (size_t)opt_int(Opt::POOL_MB, 0) << 20;
    static const size_t dflt = []() {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); total_b = size_t(128) << 30; }
        return std::min(size_t(16) << 30, total_b / 8);
    }();
    return dflt;
}
void pool_drop_locked(Pool& P, int dev) {                               // dev < 0: every device
    size_t w = 0;
    for (size_t i = 0; i < P.blocks.size(); ++i) {
        if (dev < 0 || P.blocks[i].dev == dev) { (void)hipFree(P.blocks[i].p); P.cached -= P.blocks[i].bytes; }
        else P.blocks[w++] = P.blocks[i];
    }
    P.blocks.resize(w);
}
}  // namespace

void* pool_alloc(size_t bytes, size_t* granted) {
    *granted = bytes;
    int dev = 0;
    if (bytes >= kPoolMinBytes && pool_cap_bytes() > 0) {
        ADMM_HIP_CHECK(hipGetDevice(&dev));
        Pool& P = pool();
        std::lock_guard<std::mutex> lk(P.mu);
        int best = -1;
        for (size_t i = 0; i < P.blocks.size(); ++i) {
            const PoolBlock& b = P.blocks[i];
            if (b.dev == dev && b.bytes >= bytes && b.bytes <= bytes + bytes / 4 && (best < 0 || b.bytes < P.blocks[best].bytes)) best = (int)i;
        }
        if (best >= 0) {
            void* p = P.blocks[best].p;
            *granted = P.blocks[best].bytes;
            P.cached -= P.blocks[best].bytes;
            P.blocks.erase(P.blocks.begin() + best);
            return p;
        }
    }
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) {      // give the cached blocks back and try once more
        (void)hipGetLastError();
        { Pool& P = pool(); std::lock_guard<std::mutex> lk(P.mu); pool_drop_locked(P, -1); }
        e = hipMalloc(&p, bytes);
    }
    if (e != hipSuccess)
        throw Error(ADMM_ERR_HIP, std::string("hipMalloc(") + std::to_string(bytes) + " bytes): " + hipGetErrorString(e));
    return p;
}

namespace {
thread_local std::vector<DeferredFree>* t_defer = nullptr;          // set while this thread is a rank of an in-process call
}  // namespace
void defer_frees(std::vector<DeferredFree>* sink) { t_defer = sink; }
void release_deferred(const std::vector<DeferredFree>& frees) {
    for (const DeferredFree& f : frees) { if (f.pinned) (void)hipHostFree(f.p); else pool_free(f.p, f.granted); }
}
void pinned_free(void* p) {
    if (!p) return;
    if (t_defer) { t_defer->push_back({p, 0, true}); return; }
    (void)hipHostFree(p);
}

void pool_free(void* p, size_t granted) {
    if (!p) return;
    if (t_defer) { t_defer->push_back({p, granted, false}); return; }
    if (granted >= kPoolMinBytes && pool_cap_bytes() > 0) {
        int dev = 0;
        if (hipGetDevice(&dev) == hipSuccess) {
            hipPointerAttribute_t at;
            if (hipPointerGetAttributes(&at, p) == hipSuccess) dev = at.device;      // the device the block lives on (the caller may have switched)
            Pool& P = pool();
            bool keep = false;
            {   // reserve the room first, synchronise OUTSIDE the lock (other threads' allocations must not queue behind this device's streams)
                std::lock_guard<std::mutex> lk(P.mu);
                if (P.cached + granted <= pool_cap_bytes()) { P.cached += granted; keep = true; }
            }
            if (keep) {
                // a block may be handed to another stream's work next: everything enqueued on ITS device must have finished (hipFree would
                // have waited too) -- under a device guard: the caller may have switched devices since the block was allocated
                int cur = dev;
                (void)hipGetDevice(&cur);
                if (cur != dev) (void)hipSetDevice(dev);
                (void)hipDeviceSynchronize();
                if (cur != dev) (void)hipSetDevice(cur);
                std::lock_guard<std::mutex> lk(P.mu);
                P.blocks.push_back({p, granted, dev});          // (its bytes are already counted)
                return;
            }
        }
    }
    (void)hipFree(p);
}

size_t pool_cached_bytes() {
    Pool& P = pool();
    std::lock_guard<std::mutex> lk(P.mu);
    int dev = 0;
    (void)hipGetDevice(&dev);
    size_t s = 0;
    for (const PoolBlock& b : P.blocks) if (b.dev == dev) s += b.bytes;
    return s;
}

void pool_trim() {
    Pool& P = pool();
    std::lock_guard<std::mutex> lk(P.mu);
    pool_drop_locked(P, -1);
}

}  // namespace admm
