// local_group_main.cpp -- LocalGroup and local_group_allreduce (gvamp_amd/csrc/gv_local_group.h) on their own, without HIP: rank
// threads sum messages whose magnitudes differ across the ranks, so that the order of summation shows in the bits, and every
// rank's result must be the serial rank-order sum by memcmp.  Built plain, with the address + undefined sanitizers and with the
// thread sanitizer by tests/test_host_threads_cpu.py.   exit 0 = every case held
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <thread>

#include <signal.h>
#include <unistd.h>

#include "gv_local_group.h"

namespace {
constexpr unsigned WATCHDOG_S = 600;      // a hang detector, not a measurement: 20 x the slowest thread-sanitizer run and more
constexpr int ROUNDS = 300, NLEN = 4, NVAR = 3;
constexpr size_t LENS[NLEN] = {1, 7, 4096, 100003};

uint64_t mix(uint64_t x) {      // splitmix64
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
void on_alarm(int) {
    static const char msg[] = "local_group_main: watchdog: a round did not finish\n";
    (void)!write(2, msg, sizeof(msg) - 1);
    _exit(3);
}
// message of `rank` for length index l, variant v: uniform in (-1, 1) times 10^(rank - 2), never zero
std::vector<double> message(int rank, int l, int v) {
    std::vector<double> a(LENS[l]);
    const double scale = std::pow(10.0, rank - 2);
    for (size_t i = 0; i < a.size(); i++) {
        const uint64_t h = mix(((uint64_t)rank << 48) ^ ((uint64_t)l << 40) ^ ((uint64_t)v << 32) ^ i);
        a[i] = (((double)(h >> 11) + 0.5) / 9007199254740992.0 * 2.0 - 1.0) * scale;
    }
    return a;
}
// one group of n rank threads, ROUNDS rounds; round t sends length LENS[t % 4] in variant (t / 4) % 3 -- the same on every rank
struct Run {
    int n, tag;
    gvi::LocalGroup g;
    std::vector<std::vector<double>> msg;      // [(l * NVAR + v) * n + rank]
    std::vector<std::vector<double>> want;     // [l * NVAR + v]: the serial sum in rank order, from zero
    std::atomic<int> bad{0};
    Run(int n_, int tag_) : n(n_), tag(tag_) {
        g.n = n;
        g.slots.assign((size_t)n, nullptr);
        for (int l = 0; l < NLEN; l++)
            for (int v = 0; v < NVAR; v++) {
                std::vector<double> sum(LENS[l], 0.0);
                for (int r = 0; r < n; r++) {
                    msg.push_back(message(r, l, v));
                    for (size_t i = 0; i < sum.size(); i++) sum[i] += msg.back()[i];
                }
                want.push_back(sum);
            }
    }
    void rank_thread(int rank) {
        std::vector<double> buf;      // (lives across the rounds, as the context's buffer does)
        for (int t = 0; t < ROUNDS; t++) {
            const int l = t % NLEN, v = (t / NLEN) % NVAR, k = l * NVAR + v;
            const std::vector<double>& mine = msg[(size_t)(k * n + rank)];
            buf.resize(mine.size());
            memcpy(buf.data(), mine.data(), sizeof(double) * mine.size());
            gvi::local_group_allreduce(g, rank, buf);
            if (buf.size() != mine.size() || memcmp(buf.data(), want[(size_t)k].data(), sizeof(double) * buf.size()) != 0) {
                size_t at = 0;
                while (at < buf.size() && memcmp(&buf[at], &want[(size_t)k][at], 8) == 0) at++;
                fprintf(stderr, "local_group_main: group %d of %d ranks, rank %d, round %d, %zu doubles: not the rank-order sum (first at %zu)\n",
                        tag, n, rank, t, mine.size(), at);
                bad.fetch_add(1);
                // (keep going: a rank that left would hang the others in the barrier until the watchdog)
            }
        }
    }
    void start(std::vector<std::thread>& th) {
        for (int r = 0; r < n; r++) th.emplace_back(&Run::rank_thread, this, r);
    }
};
bool run_groups(std::initializer_list<int> sizes) {
    std::vector<std::unique_ptr<Run>> runs;
    int tag = 0;
    for (int n : sizes) runs.emplace_back(new Run(n, tag++));
    std::vector<std::thread> th;
    for (auto& r : runs) r->start(th);
    for (std::thread& x : th) x.join();
    for (auto& r : runs)
        if (r->bad.load()) return false;
    return true;
}
}  // namespace

int main() {
    signal(SIGALRM, on_alarm);
    alarm(WATCHDOG_S);
    for (int n : {1, 2, 3, 8})
        if (!run_groups({n})) return 1;
    if (!run_groups({3, 2})) return 1;      // two groups at once in one process
    return 0;
}
