// gv_xfer.hip -- whole-vector transfers between the caller's host buffers and the device (to_host / to_device).  The helper
// threads that share the host's memcpy (CopyPool) live in gv_copy_pool.h, which needs no HIP and is run under the address and
// thread sanitizers by tests/test_host_threads_cpu.py.
#include "gv_copy_pool.h"
#include "gv_internal.h"

namespace gvi {

// Host <-> device transfers of whole vectors (the std::vector<double> arguments and results of data::Ax / data::ATx,
// data.hpp:117-121) through a pinned staging buffer of XFER_BYTES: a pageable user buffer costs an 8 MB copy ~5 ms on this
// runtime, a pinned one ~0.15 ms.  What is left is the host's own memcpy between the caller's buffer and the staging buffer --
// 4 MB take ~0.33 ms on one core, 15 % of a 2 ms matvec at config-2 size -- so that copy is shared among a few helper threads
// (CopyPool, gv_copy_pool.h: GV_XFER_THREADS helpers, default 3, 0 = none; they sleep between calls and spin briefly after one).
// Both functions return with the data in place.
constexpr size_t XFER_BYTES = (size_t)8 << 20;
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
