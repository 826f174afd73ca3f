// copy_pool_main.cpp -- CopyPool (gvamp_amd/csrc/gv_copy_pool.h) on its own, without HIP: every copy is compared byte for byte
// with its source and must leave the canaries on both sides of the destination alone.  One run per GV_XFER_THREADS (the pool
// reads it once).  Built plain, with the address + undefined sanitizers and with the thread sanitizer by
// tests/test_host_threads_cpu.py.   usage: copy_pool_main [--fork]      exit 0 = every case held
#include <cstdint>
#include <cstdio>

#include <signal.h>
#include <sys/wait.h>

#include "gv_copy_pool.h"

namespace {
constexpr unsigned WATCHDOG_S = 900;      // a hang detector, not a measurement: 20 x the slowest thread-sanitizer run and more
constexpr size_t KiB = 1024, MiB = 1024 * 1024;
constexpr size_t SIZES[] = {0, 1, 63, 64, 65, 256 * KiB - 1, 256 * KiB, 256 * KiB + 1, MiB + 8, 2 * MiB, 2 * MiB + 8, 8 * MiB, 8 * MiB + 24};
constexpr size_t OFFS[] = {0, 1, 8, 63};
constexpr size_t MAXN = 8 * MiB + 24, CANARY = 64;
constexpr size_t SRC_BYTES = 32 * MiB;      // every call reads another window of it, so what the destination still holds from the
                                            // call before is wrong for this one: a part left out, or copied by the previous job, shows
constexpr int HAMMER = 2000, PAUSED = 24;
std::vector<unsigned char> g_src;

uint64_t mix(uint64_t x) {      // splitmix64
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
void on_alarm(int) {
    static const char msg[] = "copy_pool_main: watchdog: a call did not return\n";
    (void)!write(2, msg, sizeof(msg) - 1);
    _exit(3);
}

struct Caller {
    int id;
    uint64_t calls = 0;
    std::vector<unsigned char> room;      // 64 spare | canary | destination | canary, at any of the start offsets
    explicit Caller(int i) : id(i), room(64 + CANARY + MAXN + CANARY + 64) {}
    // one call: false (and the case on stderr) when the bytes or a canary are wrong
    bool one(const char* what, size_t n, size_t soff, size_t doff) {
        const uint64_t k = calls++;
        const unsigned char* src = g_src.data() + (mix(k * 4 + (uint64_t)id) % (SRC_BYTES - MAXN - 64)) / 64 * 64 + soff;
        unsigned char* dst = room.data() + CANARY + doff;
        const unsigned char cv = (unsigned char)(0xC0 | (k & 0x3F));
        memset(dst - CANARY, cv, CANARY);
        memset(dst + n, cv, CANARY);
        gvi::CopyPool::get().copy(dst, src, n);
        bool ok = n == 0 || memcmp(dst, src, n) == 0;
        const char* broke = ok ? nullptr : "bytes differ";
        for (size_t i = 0; i < CANARY && !broke; i++) {
            if ((dst - CANARY)[i] != cv) broke = "canary below the destination";
            if (dst[n + i] != cv) broke = "canary above the destination";
        }
        if (!broke) return true;
        size_t at = 0;
        while (at < n && dst[at] == src[at]) at++;
        fprintf(stderr, "copy_pool_main: %s, caller %d, call %llu, n = %zu, source offset %zu, destination offset %zu: %s (first differing byte %zu)\n",
                what, id, (unsigned long long)k, n, soff, doff, broke, at);
        return false;
    }
    bool all() {
        // the grid: every size at every pair of start offsets
        for (size_t n : SIZES)
            for (size_t so : OFFS)
                for (size_t d : OFFS)
                    if (!one("grid", n, so, d)) return false;
        // back to back: the helpers are in their spin window, or still finishing the loop iteration of the previous call
        static const size_t hs[] = {256 * KiB, 256 * KiB + 1, 256 * KiB + 4096 + 65, 320 * KiB + 8};      // (just above the floor: cheap calls, many of them)
        for (int i = 0; i < HAMMER; i++)
            if (!one("back to back", hs[i % 4], OFFS[(i / 4) % 4], OFFS[(i / 16) % 4])) return false;
        // after a pause far longer than the spin window (2000 pause instructions): the helpers sleep on the condition variable
        for (int i = 0; i < PAUSED; i++) {
            usleep(3000);
            if (!one("after a pause", SIZES[5 + i % 8], OFFS[i % 4], OFFS[(i / 4) % 4])) return false;
            if (!one("behind the call after a pause", 2 * MiB, OFFS[(i + 1) % 4], OFFS[i % 4])) return false;
        }
        return true;
    }
};
}  // namespace

int main(int argc, char** argv) {
    const bool with_fork = argc > 1 && !strcmp(argv[1], "--fork");
    signal(SIGALRM, on_alarm);
    alarm(WATCHDOG_S);
    g_src.resize(SRC_BYTES);
    for (size_t i = 0; i < SRC_BYTES; i += 8) {
        const uint64_t v = mix(i / 8);
        memcpy(g_src.data() + i, &v, 8);
    }
    // one caller, then four at once (contexts of several threads share the pool: copy_mu)
    Caller first(0);
    if (!first.all()) return 1;
    {
        std::atomic<int> bad{0};
        std::vector<Caller> cs;
        for (int t = 0; t < 4; t++) cs.emplace_back(10 + t);
        std::vector<std::thread> th;
        for (int t = 1; t < 4; t++) th.emplace_back([&, t] { if (!cs[(size_t)t].all()) bad.fetch_add(1); });
        if (!cs[0].all()) bad.fetch_add(1);
        for (std::thread& x : th) x.join();
        if (bad.load()) return 1;
    }
    if (with_fork) {
        // a forked child has no helpers (threads do not survive a fork): it must copy right and return.  (This shows that such a child
        // can copy, not that the getpid() != owner rule is in force: without the rule the child would publish the jobs and take
        // every one of them itself.)
        fflush(nullptr);
        const pid_t pid = fork();
        if (pid < 0) { perror("copy_pool_main: fork"); return 2; }
        if (pid == 0) {
            alarm(WATCHDOG_S);
            Caller child(99);
            _exit(child.one("forked child", MiB, 1, 8) ? 0 : 1);
        }
        int status = 0;
        if (waitpid(pid, &status, 0) != pid || !WIFEXITED(status) || WEXITSTATUS(status) != 0) {
            fprintf(stderr, "copy_pool_main: the forked child ended with status 0x%x\n", status);
            return 1;
        }
    }
    return 0;
}
