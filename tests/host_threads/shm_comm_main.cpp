// shm_comm_main.cpp -- the process-shared transport behind GVAMP_COMM=host (gvamp_amd/csrc/host/shm_comm.cpp, linked in) on its own:
// main forks the rank processes of jobs of 2, 3 and 8 ranks before it has created any thread; the ranks meet in a segment of a
// private name, sum messages around the slot capacity and compare with the serial rank-order sum by memcmp.  Built plain and with
// the address + undefined sanitizers by tests/test_host_threads_cpu.py (not with the thread sanitizer: it cannot see another
// process's accesses to the segment).   exit 0 = every case held
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include <signal.h>
#include <sys/wait.h>
#include <unistd.h>

#include "host/shm_comm.hpp"

namespace {
constexpr unsigned WATCHDOG_S = 120;      // a hang detector, not a measurement
constexpr size_t CAP = 1000;
constexpr size_t SIZES[6] = {1, CAP - 1, CAP, CAP + 1, 3 * CAP + 7, 5};
constexpr int REPEATS = 25;

uint64_t mix(uint64_t x) {      // splitmix64
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
void on_alarm(int) {
    static const char msg[] = "shm_comm_main: watchdog: a process did not finish\n";
    (void)!write(2, msg, sizeof(msg) - 1);
    _exit(3);
}
// message k of `rank`: uniform in (-1, 1) times 10^(rank - 2), so that the order of summation shows in the bits
std::vector<double> message(int rank, int k, size_t n) {
    std::vector<double> a(n);
    const double scale = std::pow(10.0, rank - 2);
    for (size_t i = 0; i < n; i++) {
        const uint64_t h = mix(((uint64_t)rank << 48) ^ ((uint64_t)k << 32) ^ i);
        a[i] = (((double)(h >> 11) + 0.5) / 9007199254740992.0 * 2.0 - 1.0) * scale;
    }
    return a;
}
int rank_main(const std::string& name, int nranks, int rank) {
    alarm(WATCHDOG_S);
    std::string err;
    gvh_shm_comm* c = gvh_shm_open_impl(name, nranks, rank, CAP, err);
    if (!c) {
        fprintf(stderr, "shm_comm_main: %d ranks, rank %d: open failed: %s\n", nranks, rank, err.c_str());
        return 1;
    }
    int rc = 0;
    for (int k = 0; k < 6 * REPEATS && !rc; k++) {
        const size_t n = SIZES[k % 6];
        std::vector<double> want = message(0, k, n);
        for (int r = 1; r < nranks; r++) {
            const std::vector<double> a = message(r, k, n);
            for (size_t i = 0; i < n; i++) want[i] += a[i];
        }
        std::vector<double> buf = message(rank, k, n);
        if (gvh_shm_allreduce(c, buf.data(), n) != 0) {
            fprintf(stderr, "shm_comm_main: %d ranks, rank %d, message %d of %zu doubles: the all-reduce failed\n", nranks, rank, k, n);
            rc = 1;
        } else if (memcmp(buf.data(), want.data(), sizeof(double) * n) != 0) {
            size_t at = 0;
            while (memcmp(&buf[at], &want[at], 8) == 0) at++;
            fprintf(stderr, "shm_comm_main: %d ranks, rank %d, message %d of %zu doubles: not the rank-order sum (first at %zu)\n", nranks,
                    rank, k, n, at);
            rc = 1;
        }
    }
    gvh_shm_close_impl(c);
    return rc;
}
}  // namespace

int main() {
    signal(SIGALRM, on_alarm);
    alarm(WATCHDOG_S);
    int bad = 0;
    for (int nranks : {2, 3, 8}) {
        const std::string name = "/gvamp_host_threads_" + std::to_string((long)getpid()) + "_" + std::to_string(nranks);
        std::vector<pid_t> kids;
        fflush(nullptr);
        for (int r = 0; r < nranks; r++) {
            const pid_t pid = fork();
            if (pid < 0) { perror("shm_comm_main: fork"); bad++; break; }
            if (pid == 0) _exit(rank_main(name, nranks, r));
            kids.push_back(pid);
        }
        for (size_t r = 0; r < kids.size(); r++) {      // every child's exit status
            int status = 0;
            if (waitpid(kids[r], &status, 0) != kids[r] || !WIFEXITED(status) || WEXITSTATUS(status) != 0) {
                fprintf(stderr, "shm_comm_main: %d ranks: rank %zu ended with status 0x%x\n", nranks, r, status);
                bad++;
            }
        }
        if (bad) break;
    }
    return bad ? 1 : 0;
}
