// gv_local_group.h -- LocalGroup: the in-process rank group of gv_comm_init_local (gv_comm.hip), and the host half of its
// all-reduce.  Nothing of HIP in here: tests/host_threads/local_group_main.cpp compiles this header with g++ alone and runs it
// under the address and thread sanitizers ("Host-side threads under the sanitizers").
#pragma once
#include <condition_variable>
#include <cstddef>
#include <mutex>
#include <vector>

namespace gvi {

// ---- in-process communicator: nranks contexts of ONE process (threads) behave like nranks MPI ranks.  Sums in rank
// order on the host (deterministic).  For tests of the sharded algorithm on a single GPU; production uses RCCL.
struct LocalGroup {
    int n = 0;
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0;
    long gen = 0;
    std::vector<const double*> slots;
    void barrier() {
        std::unique_lock<std::mutex> lk(mu);
        const long g = gen;
        if (++arrived == n) {
            arrived = 0;
            gen++;
            cv.notify_all();
        } else
            cv.wait(lk, [&] { return gen != g; });
    }
};

// The host half of the group's SUM all-reduce, called by every rank with its own message of the same length: buf becomes the
// sum of the ranks' messages, added in rank order into a zeroed vector, so every rank holds the same bits.  The slot a rank
// published stays readable until everybody has summed (the second barrier); only then does buf change.
inline void local_group_allreduce(LocalGroup& g, int rank, std::vector<double>& buf) {
    const size_t n = buf.size();
    g.slots[rank] = buf.data();
    g.barrier();
    std::vector<double> sum(n, 0.0);
    for (int r = 0; r < g.n; r++) {
        const double* s = g.slots[r];
        for (size_t i = 0; i < n; i++) sum[i] += s[i];
    }
    g.barrier();
    buf.swap(sum);
}

}  // namespace gvi
