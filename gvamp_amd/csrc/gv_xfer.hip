// gv_xfer.hip -- whole-vector transfers between the caller's host buffers and the device (to_host / to_device).
#include <atomic>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>

#include <sched.h>
#include <unistd.h>

#include "gv_internal.h"

namespace gvi {

// Host <-> device transfers of whole vectors (the std::vector<double> arguments and results of data::Ax / data::ATx,
// data.hpp:117-121) through a pinned staging buffer of XFER_BYTES: a pageable user buffer costs an 8 MB copy ~5 ms on this
// runtime, a pinned one ~0.15 ms.  What is left is the host's own memcpy between the caller's buffer and the staging buffer --
// 4 MB take ~0.33 ms on one core, 15 % of a 2 ms matvec at config-2 size -- so that copy is shared among a few helper threads
// (CopyPool: GV_XFER_THREADS helpers, default 3, 0 = none; they sleep between calls and spin briefly after one).
// Both functions return with the data in place.
constexpr size_t XFER_BYTES = (size_t)8 << 20;
namespace {
class CopyPool {
    struct Job { char* dst; const char* src; size_t n; };
    std::vector<std::thread> th;
    std::vector<Job> jobs;
    std::unique_ptr<std::atomic<int>[]> taken;      // 1: somebody (the helper it was meant for, or the caller) has claimed job i
    std::mutex mu;
    std::condition_variable cv;
    std::atomic<unsigned long> gen{0};
    std::atomic<int> pending{0};
    bool stop = false;
    pid_t owner = 0;
    void run(int i) {
        const Job j = jobs[i];
        if (j.n) memcpy(j.dst, j.src, j.n);
        pending.fetch_sub(1, std::memory_order_acq_rel);
    }
    void work(int id) {
        unsigned long seen = 0;
        for (;;) {
            // spin a little for the next job (back-to-back matvecs), then sleep
            bool got = false;
            for (int i = 0; i < 2000 && !got; i++) {
                got = gen.load(std::memory_order_acquire) != seen;
#if defined(__x86_64__)
                if (!got) __builtin_ia32_pause();
#endif
            }
            if (!got) {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return stop || gen.load(std::memory_order_acquire) != seen; });
                if (stop) return;
            }
            seen = gen.load(std::memory_order_acquire);
            if (stop) return;
            int expect = 0;
            if (taken[id].compare_exchange_strong(expect, 1, std::memory_order_acq_rel)) run(id);   // else the caller took it
        }
    }
public:
    static CopyPool& get() {
        static CopyPool* p = new CopyPool();      // leaked on purpose: no destructor order games at process exit
        return *p;
    }
    CopyPool() {
        // helpers = min(3, CPUs this process may run on - 1); none when it has two CPUs or fewer (a cgroup of one core, several
        // ranks pinned to few cores: the caller would spin on the core its helpers need).  GV_XFER_THREADS overrides (0 = none).
        int n = 3;
        cpu_set_t cs;
        if (sched_getaffinity(0, sizeof(cs), &cs) == 0) {
            const int ncpu = CPU_COUNT(&cs);
            n = ncpu <= 2 ? 0 : (ncpu - 1 < 3 ? ncpu - 1 : 3);
        }
        if (const char* e = getenv("GV_XFER_THREADS")) n = atoi(e) < 0 ? 0 : (atoi(e) > 15 ? 15 : atoi(e));
        owner = getpid();
        jobs.assign(n, Job{nullptr, nullptr, 0});
        taken.reset(new std::atomic<int>[n > 0 ? n : 1]);
        for (int i = 0; i < n; i++) taken[i].store(1);
        try {
            for (int i = 0; i < n; i++) th.emplace_back(&CopyPool::work, this, i);
        } catch (...) {      // (no more threads to be had: the pool works with the helpers it got, copy() reads th.size())
        }
    }
    // dst <- src, n bytes, shared among the caller and the helpers (below 256 KiB, or in a forked child whose helpers did not
    // survive the fork, the caller copies alone).  Calls are serialised by copy_mu: contexts of several threads share the pool.
    // The caller never just waits: after its own part it takes over whatever a helper has not claimed yet (a helper that is
    // descheduled, or gone, cannot stall the call), and yields the core while claimed parts finish.
    std::mutex copy_mu;
    void copy(void* dst, const void* src, size_t n) {
        const int nh = (int)th.size();
        if (nh == 0 || n < ((size_t)256 << 10) || getpid() != owner) { memcpy(dst, src, n); return; }
        std::lock_guard<std::mutex> one(copy_mu);
        const size_t parts = (size_t)nh + 1, per = ((n / parts) + 63) & ~(size_t)63;
        {
            std::lock_guard<std::mutex> lk(mu);
            // Order matters: a helper still finishing its loop iteration of the PREVIOUS call may claim a job of this one the moment
            // its `taken` flag reads 0 -- so the count it will decrement is set first, and the flag is released only after the job
            // it guards has been written (the helper's claim acquires it).
            pending.store(nh, std::memory_order_relaxed);
            for (int i = 0; i < nh; i++) {
                const size_t off = per * (size_t)(i + 1);
                const size_t len = off >= n ? 0 : (i == nh - 1 ? n - off : (off + per > n ? n - off : per));
                jobs[i] = Job{(char*)dst + off, (const char*)src + off, len};
                taken[i].store(0, std::memory_order_release);
            }
            gen.fetch_add(1, std::memory_order_release);
        }
        cv.notify_all();
        memcpy(dst, src, per < n ? per : n);
        for (int i = nh - 1; i >= 0; i--) {      // work stealing, from the far end (the helpers start from their own slots)
            int expect = 0;
            if (taken[i].compare_exchange_strong(expect, 1, std::memory_order_acq_rel)) run(i);
        }
        for (unsigned long spins = 0; pending.load(std::memory_order_acquire) != 0; spins++) {
            if (spins > 4000) sched_yield();
#if defined(__x86_64__)
            else __builtin_ia32_pause();
#endif
        }
    }
};
}  // namespace
static int xfer_stage(gv_ctx* c) {
    if (!c->xfer_pin) HIPCHK(c, hipHostMalloc(&c->xfer_pin, XFER_BYTES));
    return 0;
}
int to_host(gv_ctx* c, void* dst, const void* src_dev, size_t nbytes) {
    if (xfer_stage(c)) return 1;
    // pieces of 2 MiB: the host's copy of piece k into the caller's buffer runs while pieces k + 1 ... cross PCIe (one event per
    // piece; a whole staging buffer of device-to-host copy followed by a whole buffer of memcpy cost 1.8 ms per 8 MB, of which
    // 0.3 ms were the link)
    constexpr size_t PIECE = (size_t)2 << 20;
    constexpr int NP = (int)(XFER_BYTES / PIECE);
    for (int k = 0; k < NP; k++)
        if (!c->xfer_ev[k]) HIPCHK(c, hipEventCreateWithFlags(&c->xfer_ev[k], hipEventDisableTiming));
    for (size_t off = 0; off < nbytes; off += XFER_BYTES) {
        const size_t n = nbytes - off < XFER_BYTES ? nbytes - off : XFER_BYTES;
        int np = 0;
        for (size_t q = 0; q < n; q += PIECE, np++) {
            const size_t len = n - q < PIECE ? n - q : PIECE;
            HIPCHK(c, hipMemcpyAsync((char*)c->xfer_pin + q, (const char*)src_dev + off + q, len, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipEventRecord(c->xfer_ev[np], c->stream));
        }
        np = 0;
        for (size_t q = 0; q < n; q += PIECE, np++) {
            const size_t len = n - q < PIECE ? n - q : PIECE;
            HIPCHK(c, hipEventSynchronize(c->xfer_ev[np]));
            CopyPool::get().copy((char*)dst + off + q, (char*)c->xfer_pin + q, len);
        }
    }
    if (nbytes == 0) HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
// sync = false: returns once the caller's buffer has been read (its bytes are in the staging buffer or on their way); the
// copy to the device is ordered on the context's stream like any kernel.  The next to_host / to_device synchronises the stream
// before it touches the staging buffer again.
int to_device(gv_ctx* c, void* dst_dev, const void* src, size_t nbytes, bool sync) {
    if (xfer_stage(c)) return 1;
    for (size_t off = 0; off < nbytes; off += XFER_BYTES) {
        const size_t n = nbytes - off < XFER_BYTES ? nbytes - off : XFER_BYTES;
        HIPCHK(c, hipStreamSynchronize(c->stream));       // whatever used the staging buffer last has left it
        CopyPool::get().copy(c->xfer_pin, (const char*)src + off, n);
        HIPCHK(c, hipMemcpyAsync((char*)dst_dev + off, c->xfer_pin, n, hipMemcpyHostToDevice, c->stream));
    }
    if (sync) HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

}  // namespace gvi
