// gv_capi.hip -- the core of the C ABI of include/gvamp.h over the gfx950 kernels: context lifecycle, vectors, the scalar
// mailbox, the denoiser-side entry points and instrumentation (products: gv_matvec.hip, solvers: gv_solvers.hip, data:
// gv_ingest.hip / gv_stats.hip, ranks: gv_comm.hip).  No CPU fallback anywhere: every compute entry point launches HIP
// kernels on the context's stream or fails.
#include <atomic>
#include <cassert>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <mutex>

#include "gv_internal.h"

namespace gvi {

static thread_local std::string g_create_err;

int fail(gv_ctx* c, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (c) {
        c->err = buf;
        c->pub_armed = false;          // an armed read-back whose reduction never ran must not leave read_scalars spinning
        gvk::disarm_publish();
    } else
        g_create_err = buf;
    return 1;
}

inline int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

int vec_new(gv_ctx* c, int space, gv_vec** out) {
    NEED(c, c->N > 0, "gv_set_dims must be called first");
    gv_vec* v = new gv_vec();
    v->ctx = c;
    v->space = space;
    v->len = (space == GV_SPACE_M) ? c->M : 4 * c->mbytes;
    v->cap = (space == GV_SPACE_M) ? (c->M > 0 ? c->M : 1) : c->npad;
    v->d = nullptr;
    hipError_t e = hipMalloc(&v->d, sizeof(double) * v->cap);
    if (e != hipSuccess) {
        delete v;
        return fail(c, "hipMalloc(%lld doubles) failed: %s", (long long)v->cap, hipGetErrorString(e));
    }
    e = hipMemsetAsync(v->d, 0, sizeof(double) * v->cap, c->stream);
    if (e != hipSuccess) {
        (void)hipFree(v->d);
        delete v;
        return fail(c, "hipMemsetAsync failed: %s", hipGetErrorString(e));
    }
    c->live_vecs.insert(v);
    *out = v;
    return 0;
}

int vec_need(gv_ctx* c, const char* who, const char* arg, const gv_vec* v, int space) {
    if (!v) return fail(c, "%s: %s is NULL", who, arg);
    if (v->ctx != c) return fail(c, "%s: %s belongs to another context (a gv_vec is used with the context that allocated it)", who, arg);
    if (space < 0) space = v->space;
    if (v->space != space) return fail(c, "%s: %s must be %s-space", who, arg, space == GV_SPACE_M ? "M" : "N");
    if (!vec_ok(c, v, space))
        return fail(c, "%s: %s was allocated for earlier dimensions (%lld doubles, the context now needs %lld): vectors do not outlive "
                       "gv_set_dims -- free it and allocate it again", who, arg, (long long)v->cap,
                    (long long)(space == GV_SPACE_M ? (c->M > 0 ? c->M : 1) : c->npad));
    return 0;
}

int batch_args(gv_ctx* c, const char* who, int64_t C, const gv_vec* const* in, gv_vec* const* out, const char* in_name, int in_space,
               std::vector<const double*>& is, std::vector<double*>& os) {
    const int out_space = in_space == GV_SPACE_M ? GV_SPACE_N : GV_SPACE_M;
    is.resize((size_t)C);
    os.resize((size_t)C);
    std::unordered_set<const gv_vec*> seen;
    for (int64_t j = 0; j < C; j++) {
        if (!in[j] || !out[j]) return fail(c, "%s: the handle of column %lld is NULL", who, (long long)j);
        if (in[j]->space != in_space || out[j]->space != out_space)
            return fail(c, "%s: column %lld: %s must be %s-space, out %s-space", who, (long long)j, in_name, in_space == GV_SPACE_M ? "M" : "N",
                        out_space == GV_SPACE_M ? "M" : "N");
        if (!vec_ok(c, in[j], in_space) || !vec_ok(c, out[j], out_space)) {
            const std::string w = std::string(who) + ": column " + std::to_string((long long)j);
            return vec_need(c, w.c_str(), in_name, in[j], in_space) || vec_need(c, w.c_str(), "out", out[j], out_space);
        }
        if (!seen.insert(out[j]).second) return fail(c, "%s: column %lld: two outputs are the same vector", who, (long long)j);
        is[(size_t)j] = in[j]->d;
        os[(size_t)j] = out[j]->d;
    }
    for (int64_t j = 0; j < C; j++)
        if (seen.count(in[j])) return fail(c, "%s: column %lld: an output is also an input", who, (long long)j);
    return 0;
}

int batch_host(gv_ctx* c, const char* who, int64_t C, const double* in, int in_space, bool mask_in, double* out,
               int (*dev)(gv_ctx*, int64_t, const gv_vec* const*, gv_vec* const*), double* seconds) {
    const auto t0 = std::chrono::steady_clock::now();
    const int out_space = in_space == GV_SPACE_M ? GV_SPACE_N : GV_SPACE_M;
    // Per space, whichever side it is on: a host column of M-space holds M doubles, one of N-space 4 * mbytes; an M-space column is
    // not moved when the shard has no marker (M == 0: the device vector still has one double, the host column none), an N-space
    // column always is
    auto len = [&](int space) { return space == GV_SPACE_M ? c->M : 4 * c->mbytes; };
    auto copied = [&](int space) { return space == GV_SPACE_N || c->M > 0; };
    std::vector<gv_vec*> iv, ov;
    auto drop = [&]() {
        for (gv_vec* v : iv) vec_del(c, v);
        for (gv_vec* v : ov) vec_del(c, v);
    };
    for (int64_t j = 0; j < C; j++) {
        gv_vec *a = nullptr, *b = nullptr;
        if (vec_new(c, in_space, &a)) { drop(); return 1; }
        iv.push_back(a);
        if (vec_new(c, out_space, &b)) { drop(); return 1; }
        ov.push_back(b);
        if (copied(in_space) && to_device(c, a->d, in + j * len(in_space), sizeof(double) * len(in_space), false)) { drop(); return 1; }
        if (mask_in) gvk::mask_copy(c->stream, a->d, a->d, c->mask2, c->npad);
    }
    int rc = dev(c, C, iv.data(), ov.data());
    for (int64_t j = 0; j < C && !rc && copied(out_space); j++)
        rc = to_host(c, out + j * len(out_space), ov[(size_t)j]->d, sizeof(double) * len(out_space));
    if (!rc) rc = hipStreamSynchronize(c->stream) == hipSuccess ? 0 : fail(c, "%s: hipStreamSynchronize failed", who);
    drop();
    if (!rc) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

// every gv_vec of a context goes through vec_new / vec_del, so gv_destroy can release what a caller never freed
void vec_del(gv_ctx* c, gv_vec* v) {
    if (!v) return;
    c->live_vecs.erase(v);
    if (v->owns) (void)hipFree(v->d);
    delete v;
}

// w_n and w_n2 (the N-space results of a two-vector Ax) share one allocation, w_n2 right behind w_n, so that a sharded
// job all-reduces both in ONE call (ax2_device)
int ensure_w2(gv_ctx* c) {
    if (c->w_n2) return 0;
    gv_vec* v = new gv_vec();
    *v = *c->w_n;
    v->d = c->w_n->d + c->npad;
    v->owns = false;
    c->live_vecs.insert(v);
    c->w_n2 = v;
    return 0;
}
int ensure_work(gv_ctx* c) {
    if (c->w_n && c->cg_d) {
        // free_dataset (gv_set_dims, gv_destroy) deletes every internal vector, so one that exists has the current dimensions
        assert(vec_ok(c, c->w_n, GV_SPACE_N) && vec_ok(c, c->cg_r, GV_SPACE_M) && vec_ok(c, c->cg_d, GV_SPACE_M));
        return 0;
    }
    // all or nothing: a half-built set must never be published (the entry points test w_n / cg_d and then use all five)
    gv_vec* made[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    auto undo = [&]() {
        for (gv_vec* v : made) vec_del(c, v);
        c->w_n = c->cg_r = c->cg_z = c->cg_p = c->cg_d = nullptr;
        return 1;
    };
    if (c->w_n) { vec_del(c, c->w_n); c->w_n = nullptr; }
    if (vec_new(c, GV_SPACE_N, &made[0])) return undo();
    double* both = nullptr;                                    // twice the room: w_n2 lives in the second half
    if (hipMalloc(&both, sizeof(double) * 2 * c->npad) != hipSuccess ||
        hipMemsetAsync(both, 0, sizeof(double) * 2 * c->npad, c->stream) != hipSuccess) {
        (void)hipGetLastError();
        if (both) (void)hipFree(both);
        undo();
        return fail(c, "ensure_work: no room for the N-space scratch vectors (%lld doubles)", (long long)(2 * c->npad));
    }
    (void)hipFree(made[0]->d);
    made[0]->d = both;
    for (int k = 1; k < 5; k++)
        if (vec_new(c, GV_SPACE_M, &made[k])) return undo();
    c->w_n = made[0]; c->cg_r = made[1]; c->cg_z = made[2]; c->cg_p = made[3]; c->cg_d = made[4];
    return 0;
}

// read K scalars produced by a reduction launcher back to the host.  Mailbox form (default): a one-block kernel writes
// them into mapped coherent host memory and then a sequence number; the host spins on that number -- no copy engine,
// no interrupt-driven stream synchronisation (measured: ~55 us of GPU idle per read-back with hipMemcpyAsync +
// hipStreamSynchronize, a CG step has three).  When the flag arrives every earlier kernel of the stream has finished.
void arm_scalars(gv_ctx* c) {
    if (!c->use_mbox || !c->pub_counter) return;
    c->pub_seq = ++c->mbox_seq;
    c->pub_armed = true;
    gvk::arm_publish(c->mbox_dev, reinterpret_cast<unsigned long long*>(c->mbox_dev + RED_MAXK), c->pub_seq, c->pub_counter);
}
int read_scalars(gv_ctx* c, int K, double* out) {
    if (c->use_mbox && K <= RED_MAXK) {
        unsigned long long* flag = reinterpret_cast<unsigned long long*>(c->mbox + RED_MAXK);
        unsigned long long* flag_dev = reinterpret_cast<unsigned long long*>(c->mbox_dev + RED_MAXK);
        unsigned long long seq;
        if (c->pub_armed) {            // the reduction's own finalisation publishes (arm_scalars)
            c->pub_armed = false;
            seq = c->pub_seq;
        } else {
            seq = ++c->mbox_seq;
            gvk::publish(c->stream, c->red_out, K, c->mbox_dev, flag_dev, seq);
        }
        KCHK(c);
        const auto t0 = std::chrono::steady_clock::now();
        unsigned long spins = 0;
        while (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != seq) {
            if ((++spins & 0xFFFF) == 0 &&
                std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 20.0) {
                // the kernel before it may have faulted: let the runtime say so instead of spinning for ever
                HIPCHK(c, hipStreamSynchronize(c->stream));
                if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) break;
                return fail(c, "read_scalars: the device never published the scalars");
            }
        }
        memcpy(out, c->mbox, sizeof(double) * K);
        return 0;
    }
    c->pub_armed = false;
    gvk::disarm_publish();
    HIPCHK(c, hipMemcpyAsync(c->host_pin, c->red_out, sizeof(double) * K, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    memcpy(out, c->host_pin, sizeof(double) * K);
    return 0;
}

void dense_release(gv_ctx* c, bool keep_alloc) {
    DenseData& d = c->dense;
    d.resident = d.na = false;
    d.reserved = 0;
    if (keep_alloc) return;
    for (void** q : {&d.rows, (void**)&d.mu, (void**)&d.cnt, (void**)&d.qss, (void**)&d.rcount, (void**)&d.rpart, (void**)&d.part})
        if (*q) { (void)hipFree(*q); *q = nullptr; }
    gvdm::release(d.fx);
    d.bits = 0;
    d.part_cap = 0;
}

void free_layouts(gv_ctx* c) {
    gvm::Plan& pl = c->plan;
    if (c->stripes_slab) {       // the two stripe sets are views into one allocation
        (void)hipFree(c->stripes_slab);
        c->stripes_slab = nullptr;
        pl.stripes_m = pl.stripes_n = nullptr;
    }
    for (void** q : {&pl.stripes_m, &pl.stripes_n, &pl.tiles, &pl.dig0, &pl.dig1, (void**)&pl.cv, (void**)&pl.ev, (void**)&pl.cv2,
                     (void**)&pl.ev2, (void**)&pl.scal, (void**)&pl.partial})
        if (*q) { (void)hipFree(*q); *q = nullptr; }
}

static void free_dataset(gv_ctx* c) {
    auto F = [](auto*& p) {
        if (p) (void)hipFree(p);
        p = nullptr;
    };
    F(c->bed); F(c->mask2); F(c->mave); F(c->msig); F(c->t3); F(c->ax_partial); F(c->counts);
    dense_release(c);
    free_layouts(c);
    c->score_scratch.release();
    c->atxm_scratch.release();
    c->pca_scratch.release();
    c->cov_cache.release();
    F(c->cgx_state); F(c->cgx_go);
    if (c->cgx_rel_h) (void)hipHostFree(c->cgx_rel_h);
    c->cgx_rel = c->cgx_rel_h = nullptr;
    F(c->aat_slab);
    c->aat_slab_cap = 0;
    c->cgx_relcap = 0;
    c->spec_hint_steps[0] = c->spec_hint_steps[1] = c->spec_hint_steps[2] = 0;
    c->spec_hint_passes = 0;
    c->plan = gvm::Plan();
    c->plan.deal = c->deal.ctr ? &c->deal : nullptr;
    c->have_raw = c->have_stripes = false;
    pc_invalidate(c, true);
    for (gv_vec** v : {&c->w_n, &c->cg_r, &c->cg_z, &c->cg_p, &c->cg_d, &c->mave_p, &c->msig_p, &c->numb_p, &c->w_n2,
                      &c->cg2_r, &c->cg2_z, &c->cg2_p, &c->cg2_d})
        if (*v) {
            vec_del(c, *v);
            *v = nullptr;
        }
    c->have_stats = c->have_people = false;
    cov_drop(c);
}

}  // namespace gvi

using namespace gvi;

extern "C" {

int gv_abi_version(void) { return GV_ABI_VERSION; }

// Contexts of one process (the in-process rank groups of the tests: one thread per rank) are created and torn down under one
// lock: stream / event creation and destruction racing across threads is where a runtime is least exercised, and neither
// call is on any hot path.
static std::mutex g_lifecycle_mu;
static void gv_destroy_locked(gv_ctx* c);      // the caller holds g_lifecycle_mu and has drained the streams

// The three development knobs of a batch product's kernel, <prefix>_COLS / _KS / _KERNEL: the columns per pass (one of `widths`,
// which widths_text lists for the message), the K-segments, and whether the kernel runs from one column on (1) or never (0).
// who: the entry point the messages name.  false: g_create_err says which value is refused.
static bool batch_knobs(const char* prefix, const char* who, std::initializer_list<int> widths, const char* widths_text, int& cols,
                        int& ks, int& min_cols) {
    const std::string pre(prefix);
    if (const char* sc = getenv((pre + "_COLS").c_str())) {
        char* end = nullptr;
        const long v = strtol(sc, &end, 10);
        bool ok = false;
        for (int w : widths) ok = ok || v == w;
        if (end == sc || *end != 0 || !ok) {
            g_create_err = "gv_create: " + pre + "_COLS=" + std::string(sc) + ": the columns per pass of " + who + " are " + widths_text;
            return false;
        }
        cols = (int)v;
    }
    if (const char* sk = getenv((pre + "_KS").c_str())) {
        char* end = nullptr;
        const long v = strtol(sk, &end, 10);
        if (end == sk || *end != 0 || v < 1 || v > gvm::GV_MAX_KS) {
            g_create_err = "gv_create: " + pre + "_KS=" + std::string(sk) + ": the K-segments of " + who + " are a positive integer <= " +
                           std::to_string(gvm::GV_MAX_KS);
            return false;
        }
        ks = (int)v;
    }
    if (const char* kn = getenv((pre + "_KERNEL").c_str())) min_cols = atoi(kn) != 0 ? 1 : 0x7fffffff;
    return true;
}

int gv_create(int device, gv_ctx** out) {
    if (!out) return fail(nullptr, "gv_create: out is NULL");
    *out = nullptr;
    std::lock_guard<std::mutex> life(g_lifecycle_mu);
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        return fail(nullptr, "gv_create: no HIP device available (%s); libgvamp has no CPU fallback",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device < 0 || device >= ndev) return fail(nullptr, "gv_create: device %d out of range (0..%d)", device, ndev - 1);
    gv_ctx* c = new gv_ctx();
    c->device = device;
    auto bail = [&](const char* what, hipError_t err) {
        fail(nullptr, "gv_create: %s failed: %s", what, hipGetErrorString(err));
        delete c;
        return 1;
    };
    if ((e = hipSetDevice(device)) != hipSuccess) return bail("hipSetDevice", e);
    if ((e = hipStreamCreate(&c->stream)) != hipSuccess) return bail("hipStreamCreate", e);
    if ((e = hipEventCreate(&c->ev0)) != hipSuccess) return bail("hipEventCreate", e);
    if ((e = hipEventCreate(&c->ev1)) != hipSuccess) return bail("hipEventCreate", e);
    if ((e = hipMalloc(&c->red_partial, sizeof(double) * RED_BLOCKS * RED_MAXK)) != hipSuccess) return bail("hipMalloc", e);
    if ((e = hipMalloc(&c->red_out, sizeof(double) * RED_MAXK)) != hipSuccess) return bail("hipMalloc", e);
    if ((e = hipHostMalloc(&c->host_pin, sizeof(double) * RED_MAXK)) != hipSuccess) return bail("hipHostMalloc", e);
    // scalar mailbox (read_scalars); a runtime that cannot map coherent host memory keeps the copy + synchronise read-back and the
    // host-driven CG loop
    {
        void* hp = nullptr;
        void* dp = nullptr;
        if (hipHostMalloc(&hp, sizeof(double) * RED_MAXK + 64, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess &&
            hipHostGetDevicePointer(&dp, hp, 0) == hipSuccess) {
            memset(hp, 0, sizeof(double) * RED_MAXK + 64);
            c->mbox = static_cast<double*>(hp);
            c->mbox_dev = static_cast<double*>(dp);
            c->use_mbox = true;
            if (hipMalloc(&c->pub_counter, sizeof(unsigned int)) != hipSuccess ||
                hipMemset(c->pub_counter, 0, sizeof(unsigned int)) != hipSuccess) {
                (void)hipGetLastError();
                c->pub_counter = nullptr;          // read_scalars then keeps its own publish launch
            }
        } else {
            (void)hipGetLastError();
            if (hp) (void)hipHostFree(hp);
        }
    }
    // work items of the streaming kernels dealt by ticket (gv_mfma.h).  GV_DEAL=0 (development, read per context so that one process can
    // hold both kinds): the block-index mapping.  GV_DEAL_SPARE=<d> (development): spare workgroups = items / d instead of items / 8
    {
        const char* dl = getenv("GV_DEAL");
        if (!dl || atoi(dl) != 0) {
            if ((e = hipMalloc(&c->deal.ctr, sizeof(uint32_t))) != hipSuccess) return bail("hipMalloc", e);
            if ((e = hipMemset(c->deal.ctr, 0, sizeof(uint32_t))) != hipSuccess) return bail("hipMemset", e);
            c->deal.stream = c->stream;
            c->deal.base = 0;
            if (const char* sp = getenv("GV_DEAL_SPARE")) c->deal.spare_div = atoi(sp) < 0 ? 0 : atoi(sp);
            c->plan.deal = &c->deal;
        }
    }
    // GV_DOSAGE_NA_KERNELS=1 (development, read per context as GV_DEAL is): the missing-aware dosage kernels whenever gv_set_dosage_missing
    // is on, also for a shard without a reserved code
    if (const char* nk = getenv("GV_DOSAGE_NA_KERNELS")) c->force_na_kernels = atoi(nk) != 0;
    // GV_DOSAGE_MFMA_SEG=<k> (development, read per context): most K-entries per int32 segment of the fixed-point dosage route, rounded
    // down to the kernel's K-step (at least one step).  It changes no bit; a value beyond the int32 bound is refused.
    if (const char* sg = getenv("GV_DOSAGE_MFMA_SEG")) {
        const long long k = atoll(sg);
        if (k < 1 || k > gvdm::SEG_MAX) {
            g_create_err = "gv_create: GV_DOSAGE_MFMA_SEG=" + std::string(sg) + ": a segment of the fixed-point dosage route holds 1.." +
                           std::to_string((long long)gvdm::SEG_MAX) + " K-entries (an int32 column sum gains up to 16384 per entry)";
            gv_destroy_locked(c);
            return 1;
        }
        c->dosage_seg = k;
    }
    // GV_LD_DOSAGE_EDGE=64|128 (development, read per context): the block edge of the one-product LD kernel of 8-bit dosage codes
    // (gv_set_ld_dosage).  It changes no bit.
    if (const char* ed = getenv("GV_LD_DOSAGE_EDGE")) {
        if (atoi(ed) != 64 && atoi(ed) != 128) {
            g_create_err = "gv_create: GV_LD_DOSAGE_EDGE=" + std::string(ed) + ": the block edge is 64 or 128 markers";
            gv_destroy_locked(c);
            return 1;
        }
        c->ld_dosage_edge = atoi(ed);
    }
    // GV_LD_PART_MB=<x> (development, read per context): the budget of gv_ld_scores_pos for the per-block partial sums of one pass, in MiB
    // (fractions allowed; default 2048).  It changes no bit, only the number of passes; a call whose single row group does not fit refuses.
    if (const char* pm = getenv("GV_LD_PART_MB")) {
        char* end = nullptr;
        const double mb = strtod(pm, &end);
        if (end == pm || *end != 0 || !(mb > 0.0) || !std::isfinite(mb)) {
            g_create_err = "gv_create: GV_LD_PART_MB=" + std::string(pm) + ": the budget of the LD partial sums is a positive number of MiB";
            gv_destroy_locked(c);
            return 1;
        }
        c->ld_part_bytes = mb * 1048576.0;
    }
    // GV_GRM_PART_MB=<x> (development, read per context): the budget of gv_grm_apply for the block terms of one pass, in MiB (fractions
    // allowed; default 2048).  It changes no bit, only the number of passes; a call whose single block does not fit refuses.
    if (const char* pm = getenv("GV_GRM_PART_MB")) {
        char* end = nullptr;
        const double mb = strtod(pm, &end);
        if (end == pm || *end != 0 || !(mb > 0.0) || !std::isfinite(mb)) {
            g_create_err = "gv_create: GV_GRM_PART_MB=" + std::string(pm) + ": the budget of the GRM block terms is a positive number of MiB";
            gv_destroy_locked(c);
            return 1;
        }
        c->grm_part_bytes = mb * 1048576.0;
    }
    // GV_SCORE_COLS=<4|8|16>, GV_SCORE_KS=<k>, GV_SCORE_KERNEL=1|0 and GV_ATXM_COLS=<4|8>, GV_ATXM_KS=<k>, GV_ATXM_KERNEL=1|0 (development,
    // read per context).  None changes a bit.  A GV_SCORE_KS that breaks the int32 bound on a shard is refused by the call; a
    // GV_ATXM_KS is clipped to the K-steps there are.
    if (!batch_knobs("GV_SCORE", "gv_score_dev", {4, 8, 16}, "4, 8 or 16", c->score_cols, c->score_ks, c->score_min_cols) ||
        !batch_knobs("GV_ATXM", "gv_atxm_dev", {4, 8}, "4 or 8", c->atxm_cols, c->atxm_ks, c->atxm_min_cols)) {
        gv_destroy_locked(c);
        return 1;
    }
    if (getenv("GV_ATXM_KERNEL")) c->atxm_dense_min_cols = c->atxm_min_cols;      // (1 / never, as on the bed path)
    // GV_ATXM_TILES=4|8 (development, read per context): the tiles of 16 marker rows a wave of the batch ATx kernel of 8-bit dosage codes
    // owns.  It changes no bit.
    if (const char* tl = getenv("GV_ATXM_TILES")) {
        if (strcmp(tl, "4") != 0 && strcmp(tl, "8") != 0) {
            g_create_err = "gv_create: GV_ATXM_TILES=" + std::string(tl) + ": the tiles per wave of the dosage batch kernel are 4 or 8";
            gv_destroy_locked(c);
            return 1;
        }
        c->atxm_dense_tiles = atoi(tl);
    }
    if (const char* ov = getenv("GV_OVERLAP")) c->overlap_tiles = atoi(ov) > 64 ? 64 : (atoi(ov) < 0 ? 0 : atoi(ov));
    *out = c;
    // GVAMP_FORCE_MULTI=<transport>[:<delay_us>] -- gv_debug_force_multi for every context of the process (drivers, bench.py)
    // The fault-injection bit (4) is reachable through the explicit call only, and a forced context says so once per process:
    // a job that inherits the variable must not run the loop-back transport silently.
    if (const char* fm = getenv("GVAMP_FORCE_MULTI")) {
        const int tr = atoi(fm);
        const char* colon = strchr(fm, ':');
        if (tr < 0 || tr > 3) {
            g_create_err = "gv_create: GVAMP_FORCE_MULTI=" + std::string(fm) + ": transport must be 0..3 (the fault-injection bit is gv_debug_force_multi only)";
            *out = nullptr;
            gv_destroy_locked(c);
            return 1;
        }
        if (tr > 0) {
            if (gv_debug_force_multi(c, tr, colon ? atoi(colon + 1) : 0)) {
                g_create_err = "gv_create: GVAMP_FORCE_MULTI: " + c->err;
                *out = nullptr;
                gv_destroy_locked(c);
                return 1;
            }
            static std::atomic<bool> said{false};
            if (!said.exchange(true))
                fprintf(stderr, "[gvamp] GVAMP_FORCE_MULTI=%s: one-rank contexts take the multi-rank branches over a loop-back exchange "
                                "(test hook; results are unchanged, every pass pays the exchange)\n", fm);
        }
    }
    return 0;
}

void gv_destroy(gv_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->comm_stream) (void)hipStreamSynchronize(c->comm_stream);
    std::lock_guard<std::mutex> life(g_lifecycle_mu);
    gv_destroy_locked(c);
}
static void gv_destroy_locked(gv_ctx* c) {
    c->comm = nullptr;
    c->comm_keep.reset();          // ncclCommDestroy if this was the last context sharing the communicator
    free_dataset(c);
    while (!c->live_vecs.empty()) vec_del(c, *c->live_vecs.begin());   // vectors the caller never gave back
    if (c->red_partial) (void)hipFree(c->red_partial);
    if (c->red_out) (void)hipFree(c->red_out);
    if (c->host_pin) (void)hipHostFree(c->host_pin);
    if (c->mbox) (void)hipHostFree(c->mbox);
    if (c->pub_counter) (void)hipFree(c->pub_counter);
    if (c->deal.ctr) (void)hipFree(c->deal.ctr);
    for (double* q : c->loop_buf) if (q) (void)hipFree(q);
    if (c->xfer_pin) (void)hipHostFree(c->xfer_pin);
    for (hipEvent_t e : c->xfer_ev) if (e) (void)hipEventDestroy(e);
    for (auto& r : c->ev_pool) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->ev_chunk) (void)hipEventDestroy(c->ev_chunk);
    if (c->ev_comm) (void)hipEventDestroy(c->ev_comm);
    if (c->comm_stream) { (void)hipStreamSynchronize(c->comm_stream); (void)hipStreamDestroy(c->comm_stream); }
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char* gv_last_error(const gv_ctx* c) { return c ? c->err.c_str() : g_create_err.c_str(); }

int gv_synchronize(gv_ctx* c) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // the overlapped exchange's side stream normally joins c->stream through ev_comm; a caller that synchronises wants the
    // context quiescent whatever edges were (or, under fault injection, were not) recorded
    if (c->comm_stream) HIPCHK(c, hipStreamSynchronize(c->comm_stream));
    return 0;
}

int gv_set_dims(gv_ctx* c, int64_t N, int64_t M, int64_t Mt, int64_t S) {
    NEED(c, N > 0 && M >= 0 && Mt >= M && S >= 0 && S + M <= Mt, "gv_set_dims: need N > 0, 0 <= M, S + M <= Mt");
    HIPCHK(c, hipSetDevice(c->device));
    free_dataset(c);
    c->N = N; c->M = M; c->Mt = Mt; c->S = S;
    c->mbytes = (N + 3) / 4;
    c->pitch = align_up(c->mbytes, 64);
    c->npad = 4 * c->pitch;
    c->nonas = N;
    const int64_t Mal = M > 0 ? M : 1;
    HIPCHK(c, hipMalloc(&c->mave, sizeof(double) * Mal));
    HIPCHK(c, hipMalloc(&c->msig, sizeof(double) * Mal));
    HIPCHK(c, hipMalloc(&c->t3, sizeof(double) * 3 * Mal));
    HIPCHK(c, hipMalloc(&c->counts, sizeof(uint32_t) * 3 * Mal));
    int64_t col_tiles = (c->pitch / 4 + 255) / 256;
    int64_t chunks = (2048 + col_tiles - 1) / col_tiles;
    if (chunks > 256) chunks = 256;
    if (chunks > M) chunks = M > 0 ? M : 1;
    if (chunks < 1) chunks = 1;
    c->ax_chunks = (int)chunks;
    HIPCHK(c, hipMalloc(&c->ax_partial, sizeof(double) * c->ax_chunks * c->npad));
    // i8 MFMA family: no int32 digit sum may wrap (|r'| <= 3, |digit| <= 128).  ATx side: K is the individuals, a K-entry adds at most
    // 3 * 128 and no K-segment is longer than N, so N itself is bounded here.  Ax side: K is the markers and a K-entry adds up to 512
    // (the r' plane and the miss plane share one accumulator plane); M is not bounded, the LONGEST K-segment of the decomposition is
    // (gvm::ax_bound_ok in gv_mfma.h, asked wherever a decomposition is admitted) -- only a shard that no split into 64 segments
    // can serve is refused here, on either layout
    NEED(c, N * 384 < 2147483647LL, "gv_set_dims: N too large for the int32 accumulators of kernel mode 1");
    NEED(c, gvm::ax_min_ks((M + 255) / 256, 256, M) > 0 && gvm::ax_min_ks((M + 63) / 64, 64, M) > 0,
         "gv_set_dims: M too large for the int32 accumulators of kernel mode 1 (no split into 64 K-segments keeps the Ax-side sums below 2^31)");
    // the streaming kernel counts (quad, K-block) cells in 32 bits: M N / 65536 of them (35 TB of genotypes at the limit)
    NEED(c, ((M + 255) / 256 + 1) * ((N + 255) / 256 + 1) < 2147483647LL, "gv_set_dims: shard too large for the 32-bit cell index");
    if (plan_decomps(c)) return 1;
    return gv_set_mask(c, nullptr, N);
}

int64_t gv_mbytes(const gv_ctx* c) { return c->mbytes; }

int gv_set_kernel_mode(gv_ctx* c, int mode) {
    NEED(c, mode == 0 || mode == 1 || mode == 2, "gv_set_kernel_mode: mode must be 0 (fp64 VALU), 1 (i8 MFMA fixed point) or 2 (two-level fixed point)");
    c->kernel_mode = mode;
    return 0;
}
int gv_get_kernel_mode(const gv_ctx* c) { return c->kernel_mode; }

// ---- vectors --------------------------------------------------------------------------------------------
int gv_vec_alloc(gv_ctx* c, int space, gv_vec** out) {
    NEED(c, space == GV_SPACE_M || space == GV_SPACE_N, "gv_vec_alloc: bad space");
    HIPCHK(c, hipSetDevice(c->device));
    return vec_new(c, space, out);
}
void gv_vec_free(gv_ctx* c, gv_vec* v) {
    if (!v) return;
    (void)hipStreamSynchronize(c->stream);
    vec_del(c, v);
}
int64_t gv_vec_len(const gv_vec* v) { return v->len; }
int gv_vec_upload(gv_ctx* c, gv_vec* v, const double* src) {
    NEED_VEC(c, "gv_vec_upload", v, -1);
    return to_device(c, v->d, src, sizeof(double) * (v->len > 0 ? v->len : 0));
}
int gv_vec_download(gv_ctx* c, const gv_vec* v, double* dst) {
    NEED_VEC(c, "gv_vec_download", v, -1);
    return to_host(c, dst, v->d, sizeof(double) * (v->len > 0 ? v->len : 0));
}
int gv_vec_fill(gv_ctx* c, gv_vec* v, double value) {
    NEED_VEC(c, "gv_vec_fill", v, -1);
    gvk::fill(c->stream, v->d, v->len, value);
    KCHK(c);
    return 0;
}
int gv_vec_copy(gv_ctx* c, gv_vec* dst, const gv_vec* src) {
    NEED(c, dst->space == src->space, "gv_vec_copy: space mismatch");
    NEED_VEC(c, "gv_vec_copy", dst, -1);
    NEED_VEC(c, "gv_vec_copy", src, -1);
    gvk::copy(c->stream, dst->d, src->d, src->cap);      // (a kernel: enqueued in ~3 us where hipMemcpyAsync takes the host 10-15)
    KCHK(c);
    return 0;
}
int gv_vec_axpby(gv_ctx* c, gv_vec* out, double a, const gv_vec* x, double b, const gv_vec* y) {
    NEED(c, out->space == x->space && (!y || y->space == x->space), "gv_vec_axpby: space mismatch");
    NEED(c, y || b == 0.0, "gv_vec_axpby: y is NULL but b != 0");
    NEED_VEC(c, "gv_vec_axpby", out, -1);
    NEED_VEC(c, "gv_vec_axpby", x, -1);
    NEED_VEC_OPT(c, "gv_vec_axpby", y, -1);
    gvk::axpby(c->stream, out->d, a, x->d, b, y ? y->d : nullptr, x->len);
    KCHK(c);
    return 0;
}
int gv_vec_mul(gv_ctx* c, gv_vec* out, const gv_vec* x, const gv_vec* y) {
    NEED(c, out->space == x->space && y->space == x->space, "gv_vec_mul: space mismatch");
    NEED_VEC(c, "gv_vec_mul", out, -1);
    NEED_VEC(c, "gv_vec_mul", x, -1);
    NEED_VEC(c, "gv_vec_mul", y, -1);
    gvk::mul(c->stream, out->d, x->d, y->d, x->len);
    KCHK(c);
    return 0;
}
int gv_vec_dots(gv_ctx* c, int n, const gv_vec* const* x, const gv_vec* const* y, int sync, double* out) {
    NEED(c, n >= 1 && n <= 8, "gv_vec_dots: 1 <= n <= 8");
    const double *xs[8], *ys[8];
    for (int k = 0; k < n; k++) {
        NEED(c, x[k]->space == x[0]->space && y[k]->space == x[0]->space, "gv_vec_dots: space mismatch");
        NEED_VEC(c, "gv_vec_dots", x[k], -1);
        NEED_VEC(c, "gv_vec_dots", y[k], -1);
        xs[k] = x[k]->d;
        ys[k] = y[k]->d;
    }
    if (!(sync && is_multi(c))) arm_scalars(c);
    gvk::dots(c->stream, n, xs, ys, x[0]->len, c->red_partial, c->red_out);
    KCHK(c);
    if (sync && comm_allreduce(c, c->red_out, n)) return 1;
    return read_scalars(c, n, out);
}
int gv_vec_dots_ex(gv_ctx* c, int n, const gv_dot_spec* spec, double* out) {
    NEED(c, n >= 1 && n <= 8, "gv_vec_dots_ex: 1 <= n <= 8");
    const double *xa[8], *xb[8], *ya[8], *yb[8];
    int64_t len[8];
    bool any_sync = false;
    for (int k = 0; k < n; k++) {
        const gv_dot_spec& q = spec[k];
        NEED(c, q.xa && q.ya, "gv_vec_dots_ex: xa and ya are required");
        NEED(c, q.ya->space == q.xa->space && (!q.xb || q.xb->space == q.xa->space) && (!q.yb || q.yb->space == q.xa->space),
             "gv_vec_dots_ex: the vectors of one pair live in one space");
        NEED_VEC(c, "gv_vec_dots_ex", q.xa, -1);
        NEED_VEC(c, "gv_vec_dots_ex", q.ya, -1);
        NEED_VEC_OPT(c, "gv_vec_dots_ex", q.xb, -1);
        NEED_VEC_OPT(c, "gv_vec_dots_ex", q.yb, -1);
        xa[k] = q.xa->d; xb[k] = q.xb ? q.xb->d : nullptr;
        ya[k] = q.ya->d; yb[k] = q.yb ? q.yb->d : nullptr;
        len[k] = q.xa->len;
        any_sync = any_sync || q.sync != 0;
    }
    const bool multi = any_sync && is_multi(c);
    if (!multi) arm_scalars(c);
    gvk::dots_ex(c->stream, n, xa, xb, ya, yb, len, c->red_partial, c->red_out);
    KCHK(c);
    if (multi)      // the scalars to be summed over the ranks, one all-reduce per run of neighbours
        for (int k = 0; k < n;) {
            if (!spec[k].sync) { k++; continue; }
            int e = k;
            while (e < n && spec[e].sync) e++;
            if (comm_allreduce(c, c->red_out + k, (size_t)(e - k))) return 1;
            k = e;
        }
    return read_scalars(c, n, out);
}
int gv_vec_dot(gv_ctx* c, const gv_vec* x, const gv_vec* y, int sync, double* out) {
    return gv_vec_dots(c, 1, &x, &y, sync, out);
}

int gv_set_phen(gv_ctx* c, gv_vec* y_out, const double* y_host) {
    NEED(c, y_out->space == GV_SPACE_N, "gv_set_phen: y_out must be N-space");
    NEED_VEC(c, "gv_set_phen", y_out, GV_SPACE_N);
    if (ensure_work(c)) return 1;
    std::vector<double> tmp(c->npad, 0.0);
    memcpy(tmp.data(), y_host, sizeof(double) * c->N);
    HIPCHK(c, hipMemcpyAsync(c->w_n->d, tmp.data(), sizeof(double) * c->npad, hipMemcpyHostToDevice, c->stream));
    gvk::mask_copy(c->stream, y_out->d, c->w_n->d, c->mask2, c->npad);
    KCHK(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- denoiser side ------------------------------------------------------------------------------------------
static int fill_prior(gv_ctx* c, gv_prior& pr, const double* probs, const double* vars, int L) {
    NEED(c, L >= 1 && L <= GV_LMAX, "prior: 1 <= L <= 32");
    pr.L = L;
    for (int i = 0; i < GV_LMAX; i++) {
        pr.probs[i] = i < L ? probs[i] : 0.0;
        pr.vars[i] = i < L ? vars[i] : 0.0;
    }
    return 0;
}

static int denoise_impl(gv_ctx* c, const gv_vec* r1, double gam1, const double* probs, const double* vars, int L,
                        gv_vec* x1_out, gv_vec* d_out, double* sums2, bool global) {
    NEED(c, r1->space == GV_SPACE_M && x1_out->space == GV_SPACE_M, "gv_denoise: M-space vectors required");
    NEED_VEC(c, "gv_denoise", r1, GV_SPACE_M);
    NEED_VEC(c, "gv_denoise", x1_out, GV_SPACE_M);
    NEED_VEC_OPT(c, "gv_denoise", d_out, GV_SPACE_M);
    gv_prior pr;
    if (fill_prior(c, pr, probs, vars, L)) return 1;
    const bool multi = global && is_multi(c);
    if (!multi) arm_scalars(c);
    gvk::denoise(c->stream, r1->d, c->M, gam1, pr, x1_out->d, d_out ? d_out->d : nullptr, c->red_partial, c->red_out);
    KCHK(c);
    return read_scalars_global(c, 2, sums2, multi);       // (sharded: all-reduced on the device buffer, in stream, before the read-back)
}
int gv_denoise(gv_ctx* c, const gv_vec* r1, double gam1, const double* probs, const double* vars, int L,
               gv_vec* x1_out, gv_vec* d_out, double* sums2) {
    return denoise_impl(c, r1, gam1, probs, vars, L, x1_out, d_out, sums2, false);
}
int gv_denoise_global(gv_ctx* c, const gv_vec* r1, double gam1, const double* probs, const double* vars, int L,
                      gv_vec* x1_out, gv_vec* d_out, double* sums2) {
    return denoise_impl(c, r1, gam1, probs, vars, L, x1_out, d_out, sums2, true);
}

static int prior_estep_impl(gv_ctx* c, const gv_vec* r1, double gam1, double lambda, const double* omegas,
                            const double* vars, int L, double* sums, bool global) {
    NEED(c, r1->space == GV_SPACE_M, "gv_prior_estep: M-space vector required");
    NEED_VEC(c, "gv_prior_estep", r1, GV_SPACE_M);
    NEED(c, L >= 2, "gv_prior_estep: L >= 2");
    gv_prior pr;
    if (fill_prior(c, pr, omegas, vars, L)) return 1;
    const bool multi = global && is_multi(c);
    if (!multi) arm_scalars(c);
    gvk::prior_estep(c->stream, r1->d, c->M, gam1, lambda, pr, c->red_partial, c->red_out);
    KCHK(c);
    return read_scalars_global(c, 1 + 2 * (L - 1), sums, multi);
}
int gv_prior_estep(gv_ctx* c, const gv_vec* r1, double gam1, double lambda, const double* omegas,
                   const double* vars, int L, double* sums) {
    return prior_estep_impl(c, r1, gam1, lambda, omegas, vars, L, sums, false);
}
int gv_prior_estep_global(gv_ctx* c, const gv_vec* r1, double gam1, double lambda, const double* omegas,
                          const double* vars, int L, double* sums) {
    return prior_estep_impl(c, r1, gam1, lambda, omegas, vars, L, sums, true);
}

// ---- probit: z-side denoiser of vamp::infere_bin_class (vamp_probit.cpp:335-352) -------------------------------------
int gv_probit_denoise_cov(gv_ctx* c, const gv_vec* p1, const gv_vec* y, const gv_vec* m_cov, double tau1, double probit_var,
                          gv_vec* z1_out, double* sums2) {
    NEED(c, p1->space == GV_SPACE_N && y->space == GV_SPACE_N && z1_out->space == GV_SPACE_N &&
                (!m_cov || m_cov->space == GV_SPACE_N),
         "gv_probit_denoise: N-space vectors required");
    NEED_VEC(c, "gv_probit_denoise", p1, GV_SPACE_N);
    NEED_VEC(c, "gv_probit_denoise", y, GV_SPACE_N);
    NEED_VEC(c, "gv_probit_denoise", z1_out, GV_SPACE_N);
    NEED_VEC_OPT(c, "gv_probit_denoise", m_cov, GV_SPACE_N);
    arm_scalars(c);
    gvk::probit_denoise(c->stream, p1->d, y->d, m_cov ? m_cov->d : nullptr, c->N, c->npad, tau1, probit_var, z1_out->d,
                        c->red_partial, c->red_out);
    KCHK(c);
    return read_scalars(c, 2, sums2);
}
int gv_probit_denoise(gv_ctx* c, const gv_vec* p1, const gv_vec* y, double tau1, double probit_var, gv_vec* z1_out,
                      double* sums2) {
    return gv_probit_denoise_cov(c, p1, y, nullptr, tau1, probit_var, z1_out, sums2);
}

// ---- robust: z-side denoiser and delta_H objective of vamp::infere_robust (vamp_Huber.cpp:224-260) ------------------------
// Every rank holds all N individuals: these run redundantly on each rank, with no collective.
int gv_huber_denoise(gv_ctx* c, const gv_vec* p1, const gv_vec* y, double tau1, double deltaH, gv_vec* z1_out, double* sums2) {
    NEED(c, p1 && y && z1_out && p1->space == GV_SPACE_N && y->space == GV_SPACE_N && z1_out->space == GV_SPACE_N,
         "gv_huber_denoise: N-space vectors required");
    NEED_VEC(c, "gv_huber_denoise", p1, GV_SPACE_N);
    NEED_VEC(c, "gv_huber_denoise", y, GV_SPACE_N);
    NEED_VEC(c, "gv_huber_denoise", z1_out, GV_SPACE_N);
    arm_scalars(c);
    gvk::huber_denoise(c->stream, p1->d, y->d, c->N, c->npad, tau1, deltaH, z1_out->d, c->red_partial, c->red_out);
    KCHK(c);
    return read_scalars(c, 2, sums2);
}

// log Z(d), Z(d) = int exp(-rho_d(w)) dw = sqrt(2 pi) erf(d / sqrt 2) + (2 / d) exp(-d^2 / 2): the normaliser of the Huber
// density that M_deltaH_update (vamp_Huber.cpp:554-573) leaves out
static double huber_log_norm(double d) {
    return log(sqrt(2 * M_PI) * erf(d * M_SQRT1_2) + 2.0 / d * exp(-0.5 * d * d));
}

int gv_huber_delta(gv_ctx* c, const gv_vec* p1, const gv_vec* y, double tau1, const double* grid, int G, double* obj_out) {
    NEED(c, p1 && y && p1->space == GV_SPACE_N && y->space == GV_SPACE_N, "gv_huber_delta: N-space vectors required");
    NEED_VEC(c, "gv_huber_delta", p1, GV_SPACE_N);
    NEED_VEC(c, "gv_huber_delta", y, GV_SPACE_N);
    NEED(c, grid && obj_out && G >= 1 && G <= gvk::HUBER_GMAX, "gv_huber_delta: 1 <= G <= 16 grid values required");
    gvk::HuberGrid hg{};
    for (int g = 0; g < G; g++) {
        NEED(c, grid[g] > 0 && std::isfinite(grid[g]), "gv_huber_delta: grid values must be positive and finite");
        hg.v[g] = grid[g];
    }
    NEED(c, tau1 > 0 && std::isfinite(tau1), "gv_huber_delta: tau1 must be positive and finite");
    arm_scalars(c);
    gvk::huber_delta(c->stream, p1->d, y->d, c->N, tau1, hg, G, c->red_partial, c->red_out);
    KCHK(c);
    double sums[gvk::HUBER_GMAX];
    if (read_scalars(c, G, sums)) return 1;
    for (int g = 0; g < G; g++) obj_out[g] = sums[g] / (double)c->N + huber_log_norm(grid[g]);
    return 0;
}

// ---- instrumentation ----------------------------------------------------------------------------------------------
int gv_set_timing(gv_ctx* c, int timing) {
    c->timing = timing;
    return 0;
}
int gv_get_counters(gv_ctx* c, gv_counters* out) {
    ev_resolve(c);
    *out = c->cnt;
    return 0;
}
int gv_reset_counters(gv_ctx* c) {
    ev_resolve(c);
    c->cnt = gv_counters{};
    return 0;
}
int gv_get_layout(const gv_ctx* c) {
    if (c->dense.resident) return c->dense.bits == 8 ? 4 : (c->dense.bits == 16 ? 5 : 3);
    return c->have_stripes ? (c->plan.layout == 1 ? 2 : 1) : 0;
}
int gv_copy_bandwidth(gv_ctx* c, size_t nbytes, int reps, double* gbps) {
    double *a = nullptr, *b = nullptr;
    int64_t n = (int64_t)(nbytes / 16) * 2;
    HIPCHK(c, hipMalloc(&a, n * 8));
    HIPCHK(c, hipMalloc(&b, n * 8));
    HIPCHK(c, hipMemsetAsync(a, 1, n * 8, c->stream));
    gvk::copy_bw(c->stream, a, b, n);
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    for (int i = 0; i < reps; i++) gvk::copy_bw(c->stream, a, b, n);
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, hipEventSynchronize(c->ev1));
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    *gbps = 2.0 * n * 8 * reps / (ms * 1e-3) / 1e9;
    (void)hipFree(a);
    (void)hipFree(b);
    return 0;
}

// read-only stream probe: the resident stripes when there are any (the very bytes the matvecs stream), else a scratch
// buffer of nbytes.  ~45k waves of equal contiguous runs, like a matvec launch.
int gv_read_bandwidth(gv_ctx* c, size_t nbytes, int reps, double* gbps) {
    void* buf = nullptr;
    bool own = false;
    size_t have = 0;
    if (c->have_stripes && (c->plan.stripes_m || c->plan.tiles)) {
        buf = c->plan.layout == 1 ? c->plan.tiles : c->plan.stripes_m;
        have = (size_t)c->plan.nrg_m * c->plan.nkb_m * 4096;
    }
    if (have < (size_t)64 << 20) {
        have = nbytes < ((size_t)64 << 20) ? ((size_t)64 << 20) : nbytes;
        HIPCHK(c, hipMalloc(&buf, have));
        HIPCHK(c, hipMemsetAsync(buf, 1, have, c->stream));
        own = true;
    }
    const int64_t blocks = (int64_t)(have / 4096);
    int64_t nwaves = 45056;
    if (blocks / nwaves < 16) nwaves = blocks / 16 > 0 ? blocks / 16 : 1;
    const int64_t bpw = blocks / nwaves;
    unsigned int* sink = reinterpret_cast<unsigned int*>(c->red_out);
    // lane -> piece pattern of the loads: that of the resident layout's kernels (GV_READ_PERM = 0 / 1 / 2 overrides: linear, tile
    // layout ATx side, tile layout Ax side)
    int perm = (c->have_stripes && c->plan.layout == 1) ? 1 : 0;
    if (const char* e = getenv("GV_READ_PERM")) perm = atoi(e);
    gvk::read_bw(c->stream, buf, bpw, nwaves, sink, perm);
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    for (int i = 0; i < reps; i++) gvk::read_bw(c->stream, buf, bpw, nwaves, sink, perm);
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, hipEventSynchronize(c->ev1));
    KCHK(c);
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    *gbps = (double)bpw * nwaves * 4096.0 * reps / (ms * 1e-3) / 1e9;
    if (own) (void)hipFree(buf);
    return 0;
}

}  // extern "C"
