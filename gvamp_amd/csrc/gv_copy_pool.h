// gv_copy_pool.h -- CopyPool: the helper threads that share the host's memcpy between a caller's buffer and the pinned staging
// buffer of gv_xfer.hip (to_host / to_device).  Nothing of HIP in here: tests/host_threads/copy_pool_main.cpp compiles this header
// with g++ alone and runs it under the address and thread sanitizers ("Host-side threads under the sanitizers").
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include <sched.h>
#include <sys/types.h>
#include <unistd.h>

namespace gvi {

// GV_XFER_THREADS helpers, default 3, 0 = none; they sleep between calls and spin briefly after one.
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

}  // namespace gvi
