// gv_read_slab.h -- read_slab: one slab of a file into the pinned staging buffer of gv_ingest.hip by concurrent pread streams.
// Nothing of HIP in here: tests/host_threads/read_slab_main.cpp compiles this header with g++ alone and runs it under the address
// and thread sanitizers ("Host-side threads under the sanitizers").
#pragma once
#include <cerrno>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <thread>
#include <vector>

#include <sched.h>
#include <sys/types.h>
#include <unistd.h>

namespace gvi {

// nbytes of the file at `off` into the pinned staging buffer, by GV_IO_THREADS (default 8) concurrent pread streams: one
// thread copying out of the page cache moves ~9 GB/s, a fraction of what the PCIe link takes
// returns 0 ok, -1 end of file before nbytes were read, else the errno of the failing pread (EINTR is retried)
static int read_slab(int fd, int64_t off, uint8_t* dst, size_t nbytes) {
    // 8 concurrent pread streams (measured at config-2 size out of the page cache: 4 -> 27, 8 -> 33-34, 12 -> 32-37 GB/s including
    // the allocation of the layout), never more than the CPUs this process may use
    int nt = 8;
    {
        cpu_set_t cs;
        if (sched_getaffinity(0, sizeof(cs), &cs) == 0 && CPU_COUNT(&cs) < nt) nt = CPU_COUNT(&cs) < 1 ? 1 : CPU_COUNT(&cs);
    }
    if (const char* e = getenv("GV_IO_THREADS")) nt = atoi(e) < 1 ? 1 : (atoi(e) > 32 ? 32 : atoi(e));
    if (nbytes < ((size_t)8 << 20)) nt = 1;
    std::vector<int> st(nt, 0);
    auto work = [&](int t) {
        const size_t lo = nbytes * (size_t)t / (size_t)nt, hi = nbytes * (size_t)(t + 1) / (size_t)nt;
        size_t done = lo;
        while (done < hi) {
            const ssize_t r = pread(fd, dst + done, hi - done, (off_t)(off + (int64_t)done));
            if (r < 0 && errno == EINTR) continue;
            if (r < 0) { st[t] = errno ? errno : EIO; return; }
            if (r == 0) { st[t] = -1; return; }
            done += (size_t)r;
        }
    };
    std::vector<std::thread> th;
    th.reserve((size_t)nt);
    int started = 1;                            // ranges [1, started) have a thread; the rest are read by this one
    try {
        for (; started < nt; started++) th.emplace_back(work, started);
    } catch (...) {
    }
    work(0);
    for (int t = started; t < nt; t++) work(t);
    for (std::thread& x : th) x.join();
    for (int v : st) if (v > 0) return v;      // a real I/O error wins over a short file
    for (int v : st) if (v) return v;
    return 0;
}

}  // namespace gvi
