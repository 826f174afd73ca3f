// gv_comm.hip -- the communicators of the C ABI (RCCL, the in-process rank group of the tests, the caller's host callback), the
// forced one-rank loop-back of gv_debug_force_multi, and the all-reduces of device vectors and host scalars built on them.  The
// in-process rank group (LocalGroup) and the host half of its all-reduce live in gv_local_group.h, which needs no HIP and is run
// under the address and thread sanitizers by tests/test_host_threads_cpu.py.
#include <cstring>
#include <map>
#include <memory>
#include <mutex>

#include "gv_internal.h"
#include "gv_local_group.h"

namespace gvi {

// K scalars a reduction launcher left in red_out, summed over the ranks (utilities.cpp:203) and read back: the all-reduce
// runs on the device buffer itself, so a CG scalar costs one stream synchronisation whether or not the job is sharded
int read_scalars_global(gv_ctx* c, int K, double* out, bool multi) {
    if (multi && comm_allreduce(c, c->red_out, K)) return 1;
    return read_scalars(c, K, out);
}

// MPI_Allreduce(SUM, MPI_DOUBLE) of K host scalars (utilities.cpp:203): device round trip through RCCL
int allreduce_scalars(gv_ctx* c, double* buf, int K) {
    if (!is_multi(c)) return 0;
    NEED(c, K <= RED_MAXK, "allreduce_scalars: too many scalars");
    memcpy(c->host_pin, buf, sizeof(double) * K);
    HIPCHK(c, hipMemcpyAsync(c->red_out, c->host_pin, sizeof(double) * K, hipMemcpyHostToDevice, c->stream));
    if (comm_allreduce(c, c->red_out, K)) return 1;
    return read_scalars(c, K, buf);
}

// ---- in-process communicator (gv_local_group.h): the groups of gv_comm_init_local by their number
static std::mutex g_groups_mu;
static std::map<int, std::shared_ptr<LocalGroup>> g_groups;

// (force_multi: a one-rank context made to take the sharded branches -- gv_debug_force_multi)
bool is_multi(const gv_ctx* c) { return c->force_multi != 0 || (c->nranks > 1 && (c->comm || c->local || c->cb)); }

// The exchange of a forced one-rank job: asynchronous and in-stream like RCCL's, with nothing for the host to wait on.  The
// loop-back moves the message through scratch and poisons it in between, so a consumer that is not ordered behind the exchange
// (a missing event edge between the side stream and the context's stream, a kernel enqueued ahead of its all-reduce) reads NaNs.
static int forced_allreduce(gv_ctx* c, double* dev, size_t n, hipStream_t stream) {
    if ((c->force_multi & 2) && c->comm)
        NCCLCHK(c, ncclAllReduce(dev, dev, n, ncclDouble, ncclSum, c->comm, stream));
    if (c->force_multi & 1) {
        const int q = (stream == c->stream) ? 0 : 1;
        if (c->loop_cap[q] < n) {
            // (grown once per stream to the largest message of a job, w_n | w_n2; the wait is the test hook's, not the product's)
            HIPCHK(c, hipStreamSynchronize(stream));
            if (c->loop_buf[q]) (void)hipFree(c->loop_buf[q]);
            c->loop_buf[q] = nullptr;
            c->loop_cap[q] = 0;
            const size_t cap = n > (size_t)(2 * c->npad + 64) ? n : (size_t)(2 * c->npad + 64);
            HIPCHK(c, hipMalloc(&c->loop_buf[q], sizeof(double) * cap));
            c->loop_cap[q] = cap;
        }
        gvk::loopback(stream, dev, c->loop_buf[q], (int64_t)n, c->loop_delay_us);
        KCHK(c);
    }
    return 0;
}

// SUM all-reduce of n doubles living on the device, on the context's stream
int comm_allreduce(gv_ctx* c, double* dev, size_t n) { return comm_allreduce_on(c, dev, n, c->stream); }
int comm_allreduce_on(gv_ctx* c, double* dev, size_t n, hipStream_t stream) {
    if (!is_multi(c)) return 0;
    if (c->force_multi) return forced_allreduce(c, dev, n, stream);
    if (c->comm) {
        NCCLCHK(c, ncclAllReduce(dev, dev, n, ncclDouble, ncclSum, c->comm, stream));
        return 0;
    }
    if (c->cb) {   // caller's transport (gv_comm_init_callback): host round trip
        c->local_buf.resize(n);
        HIPCHK(c, hipMemcpyAsync(c->local_buf.data(), dev, sizeof(double) * n, hipMemcpyDeviceToHost, stream));
        HIPCHK(c, hipStreamSynchronize(stream));
        if (c->cb(c->cb_user, c->local_buf.data(), n) != 0) return fail(c, "comm_allreduce: the all-reduce callback failed");
        HIPCHK(c, hipMemcpyAsync(dev, c->local_buf.data(), sizeof(double) * n, hipMemcpyHostToDevice, stream));
        HIPCHK(c, hipStreamSynchronize(stream));
        return 0;
    }
    LocalGroup* g = static_cast<LocalGroup*>(c->local);
    c->local_buf.resize(n);
    HIPCHK(c, hipMemcpyAsync(c->local_buf.data(), dev, sizeof(double) * n, hipMemcpyDeviceToHost, stream));
    HIPCHK(c, hipStreamSynchronize(stream));
    local_group_allreduce(*g, c->rank, c->local_buf);
    HIPCHK(c, hipMemcpyAsync(dev, c->local_buf.data(), sizeof(double) * n, hipMemcpyHostToDevice, stream));
    HIPCHK(c, hipStreamSynchronize(stream));
    return 0;
}

}  // namespace gvi

using namespace gvi;

extern "C" {

int gv_allreduce_host(gv_ctx* c, double* buf, int n) {
    for (int off = 0; off < n; off += RED_MAXK) {
        int k = n - off < RED_MAXK ? n - off : RED_MAXK;
        if (allreduce_scalars(c, buf + off, k)) return 1;
    }
    return 0;
}

// ---- communicator ---------------------------------------------------------------------------------------------
// the context lets go of whatever communicator it holds (the RCCL one is destroyed when its last sharer does)
static void comm_drop(gv_ctx* c) {
    c->comm = nullptr;
    c->comm_keep.reset();
    c->local = nullptr;
    c->local_keep.reset();
    c->cb = nullptr;
    c->cb_user = nullptr;
    c->rank = 0;
    c->nranks = 1;
    c->force_multi = 0;
}
int gv_comm_share(gv_ctx* c, const gv_ctx* owner) {
    NEED(c, owner != nullptr && owner != c, "gv_comm_share: owner is NULL or the context itself");
    NEED(c, owner->device == c->device || !owner->comm, "gv_comm_share: an RCCL communicator belongs to its device");
    comm_drop(c);
    c->comm = owner->comm;
    c->comm_keep = owner->comm_keep;
    c->local = owner->local;
    c->local_keep = owner->local_keep;
    c->cb = owner->cb;
    c->cb_user = owner->cb_user;
    c->rank = owner->rank;
    c->nranks = owner->nranks;
    return 0;
}
int gv_comm_unique_id(void* id128) {
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    ncclUniqueId id;
    ncclResult_t r = ncclGetUniqueId(&id);
    if (r != ncclSuccess) return fail(nullptr, "ncclGetUniqueId failed: %s", ncclGetErrorString(r));
    memcpy(id128, &id, 128);
    return 0;
}
int gv_comm_init(gv_ctx* c, int nranks, int rank, const void* id128) {
    NEED(c, nranks >= 1 && rank >= 0 && rank < nranks, "gv_comm_init: bad rank / nranks");
    HIPCHK(c, hipSetDevice(c->device));
    comm_drop(c);
    c->rank = rank;
    c->nranks = nranks;
    if (nranks == 1 && !id128) return 0;
    ncclUniqueId id;
    memcpy(&id, id128, 128);
    ncclComm_t comm = nullptr;
    NCCLCHK(c, ncclCommInitRank(&comm, nranks, id, rank));
    c->comm = comm;
    c->comm_keep = std::shared_ptr<void>(comm, [](void* p) { (void)ncclCommDestroy(static_cast<ncclComm_t>(p)); });
    // self-test: a 4-double SUM all-reduce on the context's stream must give nranks * (rank-independent value)
    double probe[4] = {1.0, 2.0, 3.0, 4.0};
    memcpy(c->host_pin, probe, sizeof(probe));
    HIPCHK(c, hipMemcpyAsync(c->red_out, c->host_pin, sizeof(probe), hipMemcpyHostToDevice, c->stream));
    NCCLCHK(c, ncclAllReduce(c->red_out, c->red_out, 4, ncclDouble, ncclSum, c->comm, c->stream));
    double back[4];
    if (read_scalars(c, 4, back)) return 1;
    for (int i = 0; i < 4; i++)
        if (back[i] != probe[i] * nranks) return fail(c, "gv_comm_init: RCCL all-reduce self-test failed (%g != %g)", back[i], probe[i] * nranks);
    return 0;
}
int gv_comm_init_local(gv_ctx* c, int group, int nranks, int rank) {
    NEED(c, nranks >= 1 && rank >= 0 && rank < nranks, "gv_comm_init_local: bad rank / nranks");
    comm_drop(c);
    std::lock_guard<std::mutex> lk(g_groups_mu);
    std::shared_ptr<LocalGroup>& g = g_groups[group];
    if (!g || g->n != nranks) {
        g = std::make_shared<LocalGroup>();
        g->n = nranks;
        g->slots.assign(nranks, nullptr);
    }
    c->local_keep = g;
    c->local = g.get();
    c->cb = nullptr;
    c->cb_user = nullptr;
    c->rank = rank;
    c->nranks = nranks;
    return 0;
}
int gv_comm_init_callback(gv_ctx* c, int nranks, int rank, gv_allreduce_fn fn, void* user) {
    NEED(c, nranks >= 1 && rank >= 0 && rank < nranks, "gv_comm_init_callback: bad rank / nranks");
    NEED(c, fn != nullptr, "gv_comm_init_callback: fn is NULL");
    comm_drop(c);
    c->cb = fn;
    c->cb_user = user;
    c->rank = rank;
    c->nranks = nranks;
    // self-test, as for RCCL: every rank must see nranks * (rank-independent value)
    double probe[4] = {1.0, 2.0, 3.0, 4.0}, back[4];
    memcpy(back, probe, sizeof(probe));
    if (nranks > 1) {
        if (allreduce_scalars(c, back, 4)) return 1;
        for (int i = 0; i < 4; i++)
            if (back[i] != probe[i] * nranks)
                return fail(c, "gv_comm_init_callback: all-reduce self-test failed (%g != %g)", back[i], probe[i] * nranks);
    }
    return 0;
}
// Test hook (include/gvamp.h): transport 0 = off, 1 = loop-back through scratch, 2 = the 1-rank RCCL communicator (created here when
// the context holds none), 3 = RCCL then the loop-back.  Only a context of a one-rank job may be forced.
int gv_debug_force_multi(gv_ctx* c, int transport, int delay_us) {
    NEED(c, transport >= 0 && transport <= 7 && (transport == 0 || (transport & 3)) && delay_us >= 0,
         "gv_debug_force_multi: transport 0..3 (+ 4: fault injection), delay_us >= 0");
    NEED(c, transport == 0 || (c->nranks == 1 && !c->local && !c->cb), "gv_debug_force_multi: only a one-rank context can be forced");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->comm_stream) HIPCHK(c, hipStreamSynchronize(c->comm_stream));     // work a dropped join (bit 4) left behind
    if ((transport & 2) && !c->comm) {
        ncclUniqueId id;
        NCCLCHK(c, ncclGetUniqueId(&id));
        if (gv_comm_init(c, 1, 0, &id)) return 1;
    }
    c->force_multi = transport;
    c->loop_delay_us = delay_us;
    return 0;
}
int gv_set_overlap(gv_ctx* c, int tiles) {
    NEED(c, tiles >= 0 && tiles <= 64, "gv_set_overlap: 0 <= tiles <= 64");
    c->overlap_tiles = tiles;
    return 0;
}
int gv_comm_rank(const gv_ctx* c) { return c->rank; }
int gv_comm_size(const gv_ctx* c) { return c->nranks; }

}  // extern "C"
