// read_slab_main.cpp -- read_slab (gvamp_amd/csrc/gv_read_slab.h) on its own, without HIP: good reads compared byte for byte with
// the file between two canaries, reads past the end of the file, and the ranking of the errors (a real errno beats a short file),
// with GV_IO_THREADS = 1, 3, 8 and 16.  Built plain, with the address + undefined sanitizers and with the thread sanitizer by
// tests/test_host_threads_cpu.py.   exit 0 = every case held
#include <cstdio>
#include <cstring>
#include <string>

#include <fcntl.h>
#include <signal.h>
#include <sys/mman.h>

#include "gv_read_slab.h"

namespace {
constexpr unsigned WATCHDOG_S = 300;      // a hang detector, not a measurement: 20 x the slowest thread-sanitizer run and more
constexpr size_t MiB = 1024 * 1024, FILE_BYTES = 24 * MiB + 17, CANARY = 64;
std::vector<uint8_t> g_want;      // the file's bytes
int g_nt = 0;

uint64_t mix(uint64_t x) {      // splitmix64
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
void on_alarm(int) {
    static const char msg[] = "read_slab_main: watchdog: a call did not return\n";
    (void)!write(2, msg, sizeof(msg) - 1);
    _exit(3);
}
bool broke(const char* what, const char* why, long a = 0, long b = 0) {
    fprintf(stderr, "read_slab_main: GV_IO_THREADS=%d, %s: %s (%ld, %ld)\n", g_nt, what, why, a, b);
    return false;
}
// a read that must succeed: the bytes of [off, off + n) between two intact canaries
bool good(int fd, const char* what, size_t off, size_t n) {
    std::vector<uint8_t> room(CANARY + n + CANARY, 0x5A);
    uint8_t* dst = room.data() + CANARY;
    memset(dst, 0xA5, n);
    const int rc = gvi::read_slab(fd, (int64_t)off, dst, n);
    if (rc != 0) return broke(what, "read_slab did not return 0", rc);
    if (memcmp(dst, g_want.data() + off, n) != 0) {
        size_t at = 0;
        while (dst[at] == g_want[off + at]) at++;
        return broke(what, "bytes differ, first at", (long)at, (long)n);
    }
    for (size_t i = 0; i < CANARY; i++)
        if (room[i] != 0x5A || dst[n + i] != 0x5A) return broke(what, "a canary was overwritten at", (long)i);
    return true;
}
// a read that must fail with `want` (-1: the file ended early, else an errno); what it did read must still stay inside dst
bool bad(int fd, const char* what, size_t off, size_t n, int want) {
    std::vector<uint8_t> room(CANARY + n + CANARY, 0x5A);
    const int rc = gvi::read_slab(fd, (int64_t)off, room.data() + CANARY, n);
    if (rc != want) return broke(what, "wrong return value (got, want)", rc, want);
    for (size_t i = 0; i < CANARY; i++)
        if (room[i] != 0x5A || room[CANARY + n + i] != 0x5A) return broke(what, "a canary was overwritten at", (long)i);
    return true;
}
}  // namespace

int main() {
    signal(SIGALRM, on_alarm);
    alarm(WATCHDOG_S);
    g_want.resize(FILE_BYTES + 8);
    for (size_t i = 0; i < FILE_BYTES; i += 8) {
        const uint64_t v = mix(i / 8);
        memcpy(g_want.data() + i, &v, 8);
    }
    g_want.resize(FILE_BYTES);
    const char* tmp = getenv("TMPDIR");
    std::string path = std::string(tmp && *tmp ? tmp : "/tmp") + "/gv_read_slab_XXXXXX";
    const int fd = mkstemp(&path[0]);
    if (fd < 0) { perror("read_slab_main: mkstemp"); return 2; }
    unlink(path.c_str());
    for (size_t done = 0; done < FILE_BYTES;) {
        const ssize_t w = write(fd, g_want.data() + done, FILE_BYTES - done);
        if (w <= 0) { perror("read_slab_main: write"); return 2; }
        done += (size_t)w;
    }
    const int closed = dup(fd);      // a descriptor number that is no longer open
    if (closed < 0) { perror("read_slab_main: dup"); return 2; }
    close(closed);
    // a destination with one page in the middle that cannot be written: pread fails there with EFAULT
    const size_t hole_bytes = FILE_BYTES + 4096;
    uint8_t* holed = (uint8_t*)mmap(nullptr, hole_bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (holed == MAP_FAILED || mprotect(holed + 12 * MiB, 4096, PROT_NONE) != 0) { perror("read_slab_main: mmap"); return 2; }

    for (int nt : {1, 3, 8, 16}) {
        g_nt = nt;
        setenv("GV_IO_THREADS", std::to_string(nt).c_str(), 1);
        if (!good(fd, "the whole file", 0, FILE_BYTES)) return 1;
        if (!good(fd, "8 MiB exactly", 3 * 4096, 8 * MiB)) return 1;
        if (!good(fd, "8 MiB - 1 (one thread)", 0, 8 * MiB - 1)) return 1;
        if (!good(fd, "unaligned offset and length", 1234567, 9 * MiB + 13)) return 1;
        if (!good(fd, "unaligned, up to the last byte of the file", 4 * MiB + 3, FILE_BYTES - (4 * MiB + 3))) return 1;
        if (!good(fd, "nothing", 5, 0)) return 1;
        if (!bad(fd, "one byte more than the file holds", 0, FILE_BYTES + 1, -1)) return 1;
        // 8 MiB that end one byte behind the file: of the nt ranges only the last one crosses the end
        if (!bad(fd, "only the last range crosses the end of the file", FILE_BYTES - 8 * MiB + 1, 8 * MiB, -1)) return 1;
        if (!bad(closed, "a closed descriptor", 0, 8 * MiB, EBADF)) return 1;
        if (!bad(closed, "a closed descriptor, one thread", 0, 4096, EBADF)) return 1;
        if (!bad(closed, "a closed descriptor and a request longer than the file", 0, FILE_BYTES + 1, EBADF)) return 1;
        // the ranges behind the hole's meet the end of the file (-1), the hole's own range fails with EFAULT: the errno is returned
        const int rc = gvi::read_slab(fd, 0, holed, hole_bytes);
        if (rc != EFAULT) return broke("an unwritable page and a request longer than the file", "wrong return value (got, want)", rc, EFAULT), 1;
    }
    munmap(holed, hole_bytes);
    close(fd);
    return 0;
}
