// gv_ingest.hip -- getting a dataset resident: PLINK .bed rows (host buffer, file, synthetic) re-encoded chunk by chunk into the
// layouts of the streaming kernels, and the rows of the dense kinds -- fp64 values of methylation data, 8- / 16-bit codes of compact
// dense data -- through one begin / copy / finish path (dense_begin, dense_finish).  The concurrent pread streams that fill a
// staging slab (read_slab) live in gv_read_slab.h, which needs no HIP and is run under the address and thread sanitizers by
// tests/test_host_threads_cpu.py.
#include <cctype>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

#include <fcntl.h>
#include <sched.h>
#include <unistd.h>

#include "gv_internal.h"
#include "gv_read_slab.h"

using namespace gvi;

extern "C" {

// Ingest: fills the resident layouts chunk by chunk (markers [m0, m0+mc), m0 % 256 == 0) so that the raw rows never
// have to be resident as a whole when only the stripes are wanted (N=400k x M=1M: 100 GB raw + 2 x 100 GB stripes).
static int ingest(gv_ctx* c, const uint8_t* host_bed, bool synth, uint64_t seed, uint32_t miss_thr, FILE* file = nullptr,
                  uint32_t ld_block = 0, uint32_t ld_thr = 0, int64_t file_off = 0) {
    NEED(c, c->N > 0, "ingest: gv_set_dims must be called first");
    NEED(c, c->want_raw || c->want_stripes, "ingest: gv_set_layout disabled both layouts");
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t M = c->M, P = c->pitch;
    gvm::Plan& pl = c->plan;
    c->have_raw = c->have_stripes = c->have_stats = c->have_people = false;
    cov_drop(c);
    pc_invalidate(c, false);      // (window Grams belong to the data set they were built from)
    dense_release(c);      // uploading any kind replaces the dataset held before
    if (c->want_raw && !c->bed) HIPCHK(c, hipMalloc(&c->bed, (size_t)(M > 0 ? M : 1) * P));
    if (!c->want_raw && c->bed) { (void)hipFree(c->bed); c->bed = nullptr; }
    const auto t_in0 = std::chrono::steady_clock::now();
    if (c->want_auto && c->want_stripes && (pl.tiles || pl.stripes_m)) {
        // a re-ingest on a context whose layout auto already picked keeps that pick: tearing a tile layout down to try two
        // stripe sets again would fail at exactly the sizes auto exists for
        c->want_tile = pl.layout == 1;
    } else if (c->want_auto && c->want_stripes) {
        // gv_set_layout(.., 3), the default: ONE tile layout -- half the bytes to allocate and fill -- unless the caller has announced a
        // long run (gv_set_expected_passes >= 1000) AND two stripe sets (the faster ATx, by 2-5 %) fit the free HBM with room for the
        // vectors and scratch.  The second set costs its bytes once more at ingest -- allocated at 25-400 GB/s depending on whether
        // the driver is still wiping freed memory, filled at ~400 GB/s: 0.5-4.3 s per 100 GB measured -- and returns ~3 % of one ATx
        // pass (bytes / 6.5 TB/s) per pass: break-even between 500 and 9 000 passes whatever the shard size (both sides scale with the
        // bytes).  A run that says nothing about its length (a bare binding, bench.py's five iterations: 5.3 of 6.4 s to solution were
        // that allocation in round 4) is not assumed to be long.
        size_t free_b = 0, total_b = 0;
        HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
        const double one = (double)((M + 63) / 64) * (double)((c->N + 255) / 256) * 4096.0;
        const double other = (c->want_raw ? (double)M * (double)P : 32768.0 * (double)P) + 64.0 * (double)(M + c->npad) + 2.0e9;
        const bool two_fit = 2.0 * one + other <= 0.92 * (double)free_b;
        c->want_tile = !(two_fit && c->expected_passes >= 1000);
    }
    const int want_layout = c->want_tile ? 1 : 0;
    const bool rebuild = c->want_stripes && (pl.layout != want_layout || !(want_layout ? pl.tiles : pl.stripes_m));
    if (rebuild) {
        // (re)build the geometry and the buffers of the MFMA family for the layout asked for
        free_layouts(c);
        if (plan_decomps(c)) return 1;
    }
    // The allocation of the resident layout -- seconds when the driver is still wiping what an earlier process freed -- runs on a
    // helper thread while this one gets the source ready: pinned staging buffers, the chunk buffer, and for a file source the
    // first two chunks read from the file system.  Wall = max(allocate, prepare) instead of their sum (gv_ingest_info2: overlap_s).
    std::string alloc_err;
    double alloc_secs = 0.0;
    auto alloc_layout = [&]() {
        const auto ta = std::chrono::steady_clock::now();
        auto A = [&](hipError_t e, const char* what) {
            if (e != hipSuccess && alloc_err.empty()) alloc_err = std::string(what) + ": " + hipGetErrorString(e);
            return e == hipSuccess;
        };
        if (!A(hipSetDevice(c->device), "hipSetDevice")) return;
        if (rebuild) {
            const int64_t nkbmax = pl.nkb_m > pl.nkb_n ? pl.nkb_m : pl.nkb_n;
            if (want_layout) {
                if (!A(hipMalloc(&pl.tiles, (size_t)(pl.nrg_m > 0 ? pl.nrg_m : 1) * pl.nkb_m * 4096), "hipMalloc(tile layout)")) return;
            } else {
                // ONE allocation for the two stripe sets, stripes_n (the Ax side) first.  Where the driver places a 100 GB allocation
                // moves the kernel that streams it by 1.5-3.5 % (docs/history/rounds1-3.md section 4.2: nine ingests on one box, Ax 14.9-15.6 ms and
                // ATx 14.8-16.0 ms from one ingest to the next); of two sets carved out of one allocation the first was in its fast
                // mode in nearly every ingest measured (Ax 14.80-14.99 ms in 13 of 14) and the second near it (ATx 14.95-15.4), whichever set
                // came first.  An allocation that large failing falls back to one allocation per set.
                const size_t sz_m = (size_t)(pl.nrg_m > 0 ? pl.nrg_m : 1) * pl.nkb_m * 4096,
                             sz_n = (size_t)pl.nrg_n * (pl.nkb_n > 0 ? pl.nkb_n : 1) * 4096;
                void* slab = nullptr;
                const size_t al = (size_t)1 << 30, off_m = (sz_n + al - 1) / al * al;
                if (hipMalloc(&slab, off_m + sz_m) == hipSuccess) {
                    c->stripes_slab = slab;
                    pl.stripes_n = slab;
                    pl.stripes_m = (char*)slab + off_m;
                } else {
                    (void)hipGetLastError();
                    if (!A(hipMalloc(&pl.stripes_m, sz_m), "hipMalloc(stripes_m)")) return;
                    if (!A(hipMalloc(&pl.stripes_n, sz_n), "hipMalloc(stripes_n)")) return;
                }
            }
            const size_t Mn = (size_t)(M > 0 ? M : 1);
            if (!A(hipMalloc(&pl.dig0, (size_t)(nkbmax > 0 ? nkbmax : 1) * 4096), "hipMalloc(dig0)")) return;
            if (!A(hipMalloc(&pl.dig1, (size_t)(nkbmax > 0 ? nkbmax : 1) * 4096), "hipMalloc(dig1)")) return;
            if (!A(hipMalloc(&pl.cv, sizeof(double) * Mn), "hipMalloc(cv)")) return;
            if (!A(hipMalloc(&pl.ev, sizeof(double) * Mn), "hipMalloc(ev)")) return;
            if (!A(hipMalloc(&pl.cv2, sizeof(double) * Mn), "hipMalloc(cv2)")) return;
            if (!A(hipMalloc(&pl.ev2, sizeof(double) * Mn), "hipMalloc(ev2)")) return;
            if (!A(hipMalloc(&pl.scal, sizeof(double) * 8), "hipMalloc(scal)")) return;
            auto pieces = [](const std::vector<gvm::Decomp>& cand, int64_t nkb) {   // room for every candidate of autotune_ks
                int k = 1;
                for (const gvm::Decomp& d : cand) {
                    const int p = (int)gvm::pieces_max(d, nkb);
                    if (p > k) k = p;
                }
                return k;
            };
            const int km = pieces(c->dec_cand_m, pl.nkb_m), kn = pieces(c->dec_cand_n, pl.nkb_n);
            size_t pa = (size_t)km * 4 * pl.nrg_m * 64 * 8 * 4, pb = (size_t)kn * 4 * pl.nrg_n * pl.rows_n * 8 * 4;
            pl.partial_bytes = pa > pb ? pa : pb;
            if (!A(hipMalloc(&pl.partial, pl.partial_bytes > 0 ? pl.partial_bytes : 4), "hipMalloc(partial sums)")) return;
        }
        alloc_secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - ta).count();
    };
    std::thread alloc_thr;
    try {
        alloc_thr = std::thread(alloc_layout);
    } catch (...) {      // (no thread to be had: allocate here, nothing overlaps)
        alloc_layout();
    }
    const auto t_prep0 = std::chrono::steady_clock::now();
    const int64_t CH = file ? 8192 : 32768;   // file source: each pinned staging buffer is CH * mbytes bytes
    uint8_t* tmp = nullptr;
    uint8_t* stage[2] = {nullptr, nullptr};
    hipEvent_t stage_free[2] = {nullptr, nullptr};
    // File source: two pinned staging buffers, so that reading chunk k + 1 from the file system overlaps the PCIe copy and the
    // re-encoding kernels of chunk k (the stream serialises the device side; an event per buffer says when its copy has left)
    int rc = 0;
    for (int b = 0; b < 2 && file && !rc; b++) {
        hipError_t e = hipHostMalloc(&stage[b], (size_t)(M < CH ? (M > 0 ? M : 1) : CH) * c->mbytes);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&stage_free[b], hipEventDisableTiming);
        if (e != hipSuccess) rc = fail(c, "ingest: no pinned staging buffer: %s", hipGetErrorString(e));
    }
    if (!c->want_raw && !rc) {
        const hipError_t e = hipMalloc(&tmp, (size_t)(M < CH ? (M > 0 ? M : 1) : CH) * P);
        if (e != hipSuccess) rc = fail(c, "ingest: no room for the chunk buffer: %s", hipGetErrorString(e));
    }
    // chunks 0 and 1 of a file come off the file system while the layout is still being allocated
    int pre_read = 0, pre_io[2] = {0, 0};
    try {
        for (int b = 0; b < 2 && file && !rc && (int64_t)b * CH < M; b++) {
            const int64_t m0 = (int64_t)b * CH, mc = M - m0 < CH ? M - m0 : CH;
            pre_io[b] = read_slab(fileno(file), file_off + m0 * c->mbytes, stage[b], (size_t)mc * c->mbytes);
            pre_read = b + 1;
        }
    } catch (const std::exception& e) {      // (no reader thread to be had: the allocation thread is still joined below)
        rc = fail(c, "ingest: reading the .bed file failed: %s", e.what());
    }
    const double prep_secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_prep0).count();
    if (alloc_thr.joinable()) alloc_thr.join();
    if (!alloc_err.empty()) {
        // nothing half-built stays behind: a retry on this context must allocate everything again (rebuild is decided from these
        // pointers), and the streaming kernels must never meet a layout whose digit / partial-sum buffers are missing
        free_layouts(c);
        (void)hipGetLastError();
        if (!rc) rc = fail(c, "ingest: allocating the resident layout failed: %s", alloc_err.c_str());
    }
    if (!rc && hipDeviceSynchronize() != hipSuccess) rc = fail(c, "ingest: hipDeviceSynchronize failed");
    const auto t_in1 = std::chrono::steady_clock::now();      // the layouts are allocated (the driver maps / wipes 100+ GB)
    c->ingest_overlap_s = alloc_secs < prep_secs ? alloc_secs : prep_secs;
    int64_t chunk = 0;
    for (int64_t m0 = 0; m0 < M && !rc; m0 += CH, chunk++) {
        const int64_t mc = M - m0 < CH ? M - m0 : CH;
        uint8_t* rawp = c->want_raw ? c->bed + m0 * P : tmp;
        hipError_t e = hipSuccess;
        const int sb = (int)(chunk & 1);
        if (synth) {
            gvk::synth_bed(c->stream, rawp, mc, c->S + m0, c->N, P, seed, miss_thr, ld_block, ld_thr);
        } else {
            const uint8_t* src = host_bed ? host_bed + (size_t)m0 * c->mbytes : stage[sb];
            if (file) {
                if (chunk >= 2) e = hipEventSynchronize(stage_free[sb]);      // the copy of chunk - 2 has left this buffer
                const int io = chunk < pre_read ? pre_io[chunk]               // (read while the layout was being allocated)
                               : (e == hipSuccess ? read_slab(fileno(file), file_off + (int64_t)m0 * c->mbytes, stage[sb], (size_t)mc * c->mbytes) : 0);
                if (io) {
                    rc = io < 0 ? fail(c, "ingest: the .bed file ends before marker %lld is complete (short file)", (long long)(c->S + m0 + mc - 1))
                                : fail(c, "ingest: reading the .bed file at marker %lld failed: %s", (long long)(c->S + m0), strerror(io));
                    break;
                }
            }
            if (e == hipSuccess) e = hipMemsetAsync(rawp, 0, (size_t)mc * P, c->stream);
            if (e == hipSuccess)
                e = hipMemcpy2DAsync(rawp, P, src, c->mbytes, c->mbytes, mc, hipMemcpyHostToDevice, c->stream);
            if (e == hipSuccess && file) e = hipEventRecord(stage_free[sb], c->stream);
        }
        if (e == hipSuccess && c->want_stripes && pl.layout == 1)
            gvm::tile_chunk(c->stream, rawp, P, mc, c->N, pl.tiles, m0 / 64, pl.nkb_m);
        else if (e == hipSuccess && c->want_stripes) {
            gvm::stripes_m_chunk(c->stream, rawp, P, mc, c->N, pl.stripes_m, m0 / 64, pl.nkb_m);
            gvm::stripes_n_chunk(c->stream, rawp, P, mc, c->N, pl.stripes_n, m0 / 256, pl.nkb_n, pl.nrg_n);
        }
        if (e == hipSuccess) e = hipGetLastError();
        // a caller-owned pageable host buffer (gv_upload_bed) and the synthetic source have nothing to overlap: keep the
        // launch queue short; the file source runs ahead by one chunk
        if (e == hipSuccess && !file) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = fail(c, "ingest chunk at marker %lld failed: %s", (long long)m0, hipGetErrorString(e));
    }
    {
        const hipError_t e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess && !rc) rc = fail(c, "ingest failed: %s", hipGetErrorString(e));
    }
    for (int b = 0; b < 2; b++) {
        if (stage[b]) (void)hipHostFree(stage[b]);
        if (stage_free[b]) (void)hipEventDestroy(stage_free[b]);
    }
    if (tmp) (void)hipFree(tmp);
    c->ingest_alloc_s = std::chrono::duration<double>(t_in1 - t_in0).count();
    c->ingest_bytes = c->want_stripes ? (size_t)(pl.layout == 1 ? 1 : 2) * (size_t)(pl.nrg_m > 0 ? pl.nrg_m : 1) * pl.nkb_m * 4096 : 0;
    if (c->want_raw) c->ingest_bytes += (size_t)(M > 0 ? M : 1) * P;
    c->ingest_fill_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_in1).count();
    if (rc) return rc;
    c->have_raw = c->want_raw;
    c->have_stripes = c->want_stripes;
    return 0;
}

int gv_set_layout(gv_ctx* c, int raw_rows, int stripes) {
    NEED(c, raw_rows || stripes, "gv_set_layout: at least one layout is required");
    NEED(c, stripes >= 0 && stripes <= 3, "gv_set_layout: stripes is 0 (none), 1 (two stripe sets), 2 (one tile layout) or 3 (auto)");
    c->want_raw = raw_rows != 0;
    c->want_stripes = stripes != 0;
    c->want_tile = stripes == 2;
    c->want_auto = stripes == 3;
    return 0;
}

int gv_upload_bed(gv_ctx* c, const uint8_t* bed, size_t nbytes) {
    NEED(c, c->N > 0, "gv_upload_bed: gv_set_dims must be called first");
    NEED(c, nbytes == (size_t)c->M * (size_t)c->mbytes, "gv_upload_bed: nbytes != M * ceil(N/4)");
    return ingest(c, bed, false, 0, 0);
}

int gv_upload_bed_file(gv_ctx* c, const char* path, int64_t offset) {
    NEED(c, c->N > 0, "gv_upload_bed_file: gv_set_dims must be called first");
    FILE* f = fopen(path, "rb");
    if (!f) return fail(c, "gv_upload_bed_file: could not open bed file: %s", path);
    if (fseeko(f, (off_t)offset, SEEK_SET) != 0) {
        fclose(f);
        return fail(c, "gv_upload_bed_file: cannot seek to %lld in %s", (long long)offset, path);
    }
    int rc = ingest(c, nullptr, false, 0, 0, f, 0, 0, offset);
    fclose(f);
    return rc;
}

int gv_synth_bed(gv_ctx* c, uint64_t seed, uint32_t miss_ppm) {
    NEED(c, c->N > 0, "gv_synth_bed: gv_set_dims must be called first");
    uint32_t thr = (uint32_t)(((uint64_t)miss_ppm << 32) / 1000000ull);
    return ingest(c, nullptr, true, seed, thr);
}

int gv_synth_bed_ld(gv_ctx* c, uint64_t seed, uint32_t miss_ppm, uint32_t ld_block, uint32_t ld_ppm) {
    NEED(c, c->N > 0, "gv_synth_bed_ld: gv_set_dims must be called first");
    NEED(c, ld_ppm <= 1000000, "gv_synth_bed_ld: ld_ppm is a probability in 1e-6");
    const uint32_t thr = (uint32_t)(((uint64_t)miss_ppm << 32) / 1000000ull);
    const uint64_t lt = ((uint64_t)ld_ppm << 32) / 1000000ull;
    return ingest(c, nullptr, true, seed, thr, nullptr, ld_block, (uint32_t)(lt > 0xFFFFFFFFull ? 0xFFFFFFFFull : lt));
}

// ---- the dense kinds: the fp64 design matrix of methylation data (type_data == "meth") and the code rows of compact dense data ----
// An upload runs between dense_begin and dense_finish; the clock carries its start and the seconds the allocation took.
struct DenseClock {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double alloc_s = 0.0;
};
// Frees whatever genotype layout is resident (the next bed ingest rebuilds it) and allocates the dense rows, zeroed.
// bits: 0 = fp64 values, 8 / 16 = unsigned codes, X = scale * B (the mean codes of the statistics get their M doubles here too)
static int dense_begin(gv_ctx* c, int bits, double scale, DenseClock* clk) {
    NEED(c, c->N > 0, "dense upload: gv_set_dims must be called first");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    free_layouts(c);
    if (c->bed) { (void)hipFree(c->bed); c->bed = nullptr; }
    c->have_raw = c->have_stripes = c->have_stats = c->have_people = false;
    cov_drop(c);
    pc_invalidate(c, false);        // (window Grams belong to the data set they were built from)
    c->ingest_bytes = 0;
    DenseData& d = c->dense;
    dense_release(c, bits == d.bits && d.rows);      // rows of this width are held: their allocation is used again
    if (!d.cus) {
        int cus = 0;
        HIPCHK(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
        d.cus = cus > 0 ? cus : 256;
    }
    const size_t rows = (size_t)(c->M > 0 ? c->M : 1);
    d.pitch = gvd::row_pitch(c->N);
    if (!d.rows) {      // another width (or nothing) was held: allocate afresh
        d.bits = bits;
        hipError_t e = hipMalloc(&d.rows, d.bytes((int64_t)rows));
        if (e == hipSuccess && bits) e = hipMalloc(&d.mu, sizeof(double) * rows);
        if (e == hipSuccess && bits) e = hipMalloc(&d.cnt, sizeof(double) * rows);
        if (e == hipSuccess && bits) e = hipMalloc(&d.qss, sizeof(double) * rows);
        if (e != hipSuccess) {
            dense_release(c);
            return fail(c, "dense upload: no room for %lld x %lld %s in HBM: %s", (long long)c->M, (long long)d.pitch,
                        bits == 8 ? "8-bit codes" : (bits == 16 ? "16-bit codes" : "doubles"), hipGetErrorString(e));
        }
    }
    d.scale = scale;
    HIPCHK(c, hipMemsetAsync(d.rows, 0, d.bytes((int64_t)rows), c->stream));
    if (bits && c->dosage_missing) {      // the count of reserved codes of this upload starts at zero (count_reserved)
        if (!d.rcount) HIPCHK(c, hipMalloc(&d.rcount, sizeof(unsigned long long)));
        if (!d.rpart) HIPCHK(c, hipMalloc(&d.rpart, sizeof(unsigned long long) * gvd::COUNT_BLOCKS));
        HIPCHK(c, hipMemsetAsync(d.rcount, 0, sizeof(unsigned long long), c->stream));
    }
    clk->alloc_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - clk->t0).count();
    return 0;
}
// gv_set_dosage_missing: the reserved codes of the pitched rows [m0, m0 + mc), counted on the device behind their copy
static void count_reserved(gv_ctx* c, int64_t m0, int64_t mc) {
    if (!c->dosage_missing || !c->dense.bits || mc <= 0) return;
    gvd::count_reserved(c->stream, dense_view(c), m0, mc, c->dense.rpart, c->dense.rcount);
}
static int dense_finish(gv_ctx* c, const DenseClock& clk) {
    DenseData& d = c->dense;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (d.bits && c->dosage_missing) {
        HIPCHK(c, hipMemcpy(&d.reserved, d.rcount, sizeof(unsigned long long), hipMemcpyDeviceToHost));
        d.na = true;
    }
    c->ingest_alloc_s = clk.alloc_s;
    c->ingest_overlap_s = 0.0;
    c->ingest_fill_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - clk.t0).count() - clk.alloc_s;
    c->ingest_bytes = d.bytes(c->M);
    d.resident = true;
    return 0;
}
// M * N elements of a caller-owned pageable host buffer into the pitched rows, `step` rows per copy (nothing to overlap)
static int dense_copy_host(gv_ctx* c, const void* src, int64_t step) {
    const DenseData& d = c->dense;
    const size_t rowb = d.elem_bytes() * (size_t)c->N, pitchb = d.elem_bytes() * (size_t)d.pitch;
    const int64_t rows = c->M < step ? c->M : step;
    for (int64_t m0 = 0; m0 < c->M; m0 += rows) {
        const int64_t mc = c->M - m0 < rows ? c->M - m0 : rows;
        HIPCHK(c, hipMemcpy2DAsync((char*)d.rows + (size_t)m0 * pitchb, pitchb, (const char*)src + (size_t)m0 * rowb, rowb, rowb, mc,
                                   hipMemcpyHostToDevice, c->stream));
        count_reserved(c, m0, mc);
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return 0;
}

int gv_upload_meth(gv_ctx* c, const double* x, size_t n) {
    NEED(c, c->N > 0, "gv_upload_meth: gv_set_dims must be called first");
    NEED(c, n == (size_t)c->M * (size_t)c->N, "gv_upload_meth: n != M * N");
    DenseClock clk;
    if (dense_begin(c, 0, 1.0, &clk) || dense_copy_host(c, x, 4096)) return 1;
    return dense_finish(c, clk);
}

// read_methylation_data (data.cpp:241-278): M*N doubles at byte `offset` (= S*N*8, :259), streamed through two bounded pinned
// buffers as gv_upload_bed_file streams a .bed: reading chunk k + 1 overlaps the copy of chunk k, host memory stays O(chunk).
// (shared with gv_upload_dosage_file: bits = 0 reads doubles, 8 / 16 reads codes of that width; `who` names the entry point)
static int dense_upload_file(gv_ctx* c, const char* who, const char* path, int64_t offset, int bits, double scale) {
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return fail(c, "%s: could not open %s file: %s", who, bits ? "dosage" : "methylation", path);
    DenseClock clk;
    int rc = dense_begin(c, bits, scale, &clk);
    const size_t esz = bits ? (size_t)bits / 8 : sizeof(double);
    const size_t rowb = esz * (size_t)c->N, pitchb = esz * (size_t)c->dense.pitch;
    char* const dst = (char*)c->dense.rows;
    int64_t CH = (int64_t)(((size_t)64 << 20) / rowb);
    if (CH < 1) CH = 1;
    if (CH > c->M) CH = c->M > 0 ? c->M : 1;
    void* stage[2] = {nullptr, nullptr};
    hipEvent_t stage_free[2] = {nullptr, nullptr};
    for (int b = 0; b < 2 && !rc; b++) {
        hipError_t e = hipHostMalloc(&stage[b], (size_t)CH * rowb);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&stage_free[b], hipEventDisableTiming);
        if (e != hipSuccess) rc = fail(c, "%s: no pinned staging buffer: %s", who, hipGetErrorString(e));
    }
    int64_t chunk = 0;
    for (int64_t m0 = 0; m0 < c->M && !rc; m0 += CH, chunk++) {
        const int64_t mc = c->M - m0 < CH ? c->M - m0 : CH;
        const int sb = (int)(chunk & 1);
        hipError_t e = hipSuccess;
        if (chunk >= 2) e = hipEventSynchronize(stage_free[sb]);      // the copy of chunk - 2 has left this buffer
        if (e != hipSuccess) { rc = fail(c, "%s: %s", who, hipGetErrorString(e)); break; }
        const int io = read_slab(fd, offset + m0 * (int64_t)rowb, (uint8_t*)stage[sb], (size_t)mc * rowb);
        if (io) {
            rc = io < 0 ? fail(c, "%s: %s ends before marker %lld is complete (short file)", who, path, (long long)(c->S + m0 + mc - 1))
                        : fail(c, "%s: reading %s at marker %lld failed: %s", who, path, (long long)(c->S + m0), strerror(io));
            break;
        }
        e = hipMemcpy2DAsync(dst + (size_t)m0 * pitchb, pitchb, stage[sb], rowb, rowb, mc, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipEventRecord(stage_free[sb], c->stream);
        if (e == hipSuccess && bits) count_reserved(c, m0, mc);
        if (e != hipSuccess) rc = fail(c, "%s: copy at marker %lld failed: %s", who, (long long)(c->S + m0), hipGetErrorString(e));
    }
    (void)hipStreamSynchronize(c->stream);
    for (int b = 0; b < 2; b++) {
        if (stage[b]) (void)hipHostFree(stage[b]);
        if (stage_free[b]) (void)hipEventDestroy(stage_free[b]);
    }
    close(fd);
    if (rc) return rc;
    return dense_finish(c, clk);
}

int gv_upload_meth_file(gv_ctx* c, const char* path, int64_t offset) {
    NEED(c, c->N > 0, "gv_upload_meth_file: gv_set_dims must be called first");
    NEED(c, offset >= 0, "gv_upload_meth_file: negative offset");
    return dense_upload_file(c, "gv_upload_meth_file", path, offset, 0, 1.0);
}

int gv_synth_meth(gv_ctx* c, uint64_t seed) {
    NEED(c, c->N > 0, "gv_synth_meth: gv_set_dims must be called first");
    DenseClock clk;
    if (dense_begin(c, 0, 1.0, &clk)) return 1;
    gvd::synth(c->stream, dense_view(c), c->S, seed);
    KCHK(c);
    return dense_finish(c, clk);
}

// ---- compact dense data: X = scale * B, B unsigned codes of 8 or 16 bits (gv_dense.hip: k_dosage_*) ------------------------------
static int dosage_args(gv_ctx* c, const char* who, int bits, double scale) {
    if (c->N <= 0) return fail(c, "%s: gv_set_dims must be called first", who);
    if (bits != 8 && bits != 16) return fail(c, "%s: bits must be 8 or 16, not %d", who, bits);
    if (!(scale > 0.0) || !std::isfinite(scale)) return fail(c, "%s: scale must be positive and finite, not %g", who, scale);
    return 0;
}

int gv_upload_dosage(gv_ctx* c, const void* codes, size_t n, int bits, double scale) {
    if (dosage_args(c, "gv_upload_dosage", bits, scale)) return 1;
    NEED(c, n == (size_t)c->M * (size_t)c->N, "gv_upload_dosage: n != M * N");
    DenseClock clk;
    if (dense_begin(c, bits, scale, &clk) || dense_copy_host(c, codes, 16384)) return 1;
    KCHK(c);
    return dense_finish(c, clk);
}

// M*N codes at byte `offset` (= S*N*bits/8), streamed through the two bounded pinned buffers of gv_upload_meth_file
int gv_upload_dosage_file(gv_ctx* c, const char* path, int64_t offset, int bits, double scale) {
    if (dosage_args(c, "gv_upload_dosage_file", bits, scale)) return 1;
    NEED(c, offset >= 0, "gv_upload_dosage_file: negative offset");
    return dense_upload_file(c, "gv_upload_dosage_file", path, offset, bits, scale);
}

static int synth_dosage(gv_ctx* c, uint64_t seed, int bits, bool na, uint64_t miss_thr, uint64_t ld_block = 0, uint64_t ld_thr = 0) {
    DenseClock clk;
    if (dense_begin(c, bits, bits == 8 ? 1.0 / 127.0 : 1.0 / 16384.0, &clk)) return 1;
    gvd::View v = dense_view(c);
    v.na = na;      // (of the generator: nothing is resident yet)
    if (ld_block) gvd::synth_ld(c->stream, v, c->S, seed, miss_thr, ld_block, ld_thr);
    else gvd::synth(c->stream, v, c->S, seed, miss_thr);
    count_reserved(c, 0, c->M);
    KCHK(c);
    return dense_finish(c, clk);
}

int gv_synth_dosage(gv_ctx* c, uint64_t seed, int bits) {
    if (dosage_args(c, "gv_synth_dosage", bits, 1.0)) return 1;
    return synth_dosage(c, seed, bits, false, 0);
}

int gv_synth_dosage_na(gv_ctx* c, uint64_t seed, int bits, uint32_t miss_ppm) {
    if (dosage_args(c, "gv_synth_dosage_na", bits, 1.0)) return 1;
    NEED(c, miss_ppm <= 1000000u, "gv_synth_dosage_na: miss_ppm above 1000000");
    c->dosage_missing = true;      // (the data set held before is replaced: nothing resident goes stale)
    return synth_dosage(c, seed, bits, true, ((uint64_t)miss_ppm << 32) / 1000000ull);
}

int gv_synth_dosage_ld(gv_ctx* c, uint64_t seed, int bits, uint32_t miss_ppm, uint32_t ld_block, uint32_t ld_ppm) {
    if (dosage_args(c, "gv_synth_dosage_ld", bits, 1.0)) return 1;
    NEED(c, miss_ppm <= 1000000u, "gv_synth_dosage_ld: miss_ppm above 1000000");
    NEED(c, ld_ppm <= 1000000u, "gv_synth_dosage_ld: ld_ppm is a probability in 1e-6");
    NEED(c, ld_block >= 1, "gv_synth_dosage_ld: ld_block must be at least 1 marker");
    if (miss_ppm) c->dosage_missing = true;      // (reserved codes are written: they are missing entries, as gv_synth_dosage_na's)
    const uint64_t lt = ((uint64_t)ld_ppm << 32) / 1000000ull;
    return synth_dosage(c, seed, bits, false, ((uint64_t)miss_ppm << 32) / 1000000ull, ld_block, lt > 0xFFFFFFFFull ? 0xFFFFFFFFull : lt);
}

int gv_set_dosage_missing(gv_ctx* c, int on) {
    const bool want = on != 0;
    if (c->dense.resident && c->dense.bits && want != c->dense.na)
        return fail(c, "gv_set_dosage_missing: %d-bit codes are resident and were uploaded with the option %s; their statistics would be "
                       "stale -- set it before the upload", c->dense.bits, c->dense.na ? "on" : "off");
    if (want != c->dosage_missing) pc_invalidate(c, false);
    c->dosage_missing = want;
    return 0;
}

int gv_set_dosage_route(gv_ctx* c, int route) {
    NEED(c, route == 0 || route == 1, "gv_set_dosage_route: route must be 0 (VALU kernels) or 1 (fixed-point i8 MFMA)");
    c->dosage_route = route;
    return 0;
}

int gv_get_dosage_route(const gv_ctx* c, int* requested, int* in_force) {
    if (requested) *requested = c->dosage_route;
    if (in_force) *in_force = dosage_mfma_route(c) ? 1 : 0;
    return 0;
}

int gv_dosage_info(gv_ctx* c, gv_dosage_stats* out) {
    NEED(c, out != nullptr, "gv_dosage_info: out is NULL");
    const DenseData& d = c->dense;
    const bool res = d.resident && d.bits;
    out->bits = res ? d.bits : 0;
    out->scale = res ? d.scale : 0.0;
    out->missing = (res ? d.na : c->dosage_missing) ? 1 : 0;
    out->reserved = res ? (uint64_t)d.reserved : 0;
    out->na_kernels = res && dosage_na_kernels(c) ? 1 : 0;
    out->pad_ = 0;
    return 0;
}

int gv_download_bed(gv_ctx* c, uint8_t* bed, size_t nbytes) {
    REFUSE_DOSAGE(c, "gv_download_bed", "the resident dataset is a matrix of dosage codes, not PLINK rows");
    NEED(c, !c->dense.resident, "gv_download_bed: the resident dataset is methylation data (a dense fp64 matrix), not PLINK rows");
    NEED(c, c->have_raw, "gv_download_bed: the raw row layout is not resident (not the default: call gv_set_layout(ctx, 1, stripes) before the ingest)");
    NEED(c, nbytes == (size_t)c->M * (size_t)c->mbytes, "gv_download_bed: nbytes != M * ceil(N/4)");
    if (c->M > 0)
        HIPCHK(c, hipMemcpy2DAsync(bed, c->mbytes, c->bed, c->pitch, c->mbytes, c->M, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int gv_ingest_info(gv_ctx* c, double* alloc_seconds, double* fill_seconds) {
    if (alloc_seconds) *alloc_seconds = c->ingest_alloc_s;
    if (fill_seconds) *fill_seconds = c->ingest_fill_s;
    return 0;
}
// The calling thread (and the threads it starts afterwards: the staging-copy helpers, the file readers) is restricted to the CPUs of
// the NUMA node the GPU hangs off -- /sys/bus/pci/devices/<bus id>/numa_node and /sys/devices/system/node/node<k>/cpulist --
// intersected with the CPUs it may already run on.  The host-paced sections of a VAMP iteration and the pinned staging copies
// cross the socket interconnect otherwise (18.9 % idle measured on a box whose host was the far socket).
int gv_bind_host_numa(int device, int* numa_node_out) {
    if (numa_node_out) *numa_node_out = -1;
    if (const char* e = getenv("GVAMP_NUMA_BIND"))
        if (atoi(e) == 0) return 0;
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), device) != hipSuccess) { (void)hipGetLastError(); return fail(nullptr, "gv_bind_host_numa: no PCI bus id for device %d", device); }
    for (char* q = bus; *q; q++) *q = (char)tolower((unsigned char)*q);
    char path[256];
    snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bus);
    FILE* f = fopen(path, "r");
    int node = -1;
    if (f) { if (fscanf(f, "%d", &node) != 1) node = -1; fclose(f); }
    if (node < 0) return 0;                       // a single-node host (or a VM that hides the topology): nothing to do
    snprintf(path, sizeof(path), "/sys/devices/system/node/node%d/cpulist", node);
    f = fopen(path, "r");
    if (!f) return 0;
    char list[4096] = {0};
    const bool got = fgets(list, sizeof(list), f) != nullptr;
    fclose(f);
    if (!got) return 0;
    cpu_set_t want, have, both;
    CPU_ZERO(&want);
    for (char* q = list; *q;) {                   // "0-15,128-143"
        char* end = nullptr;
        const long a = strtol(q, &end, 10);
        if (end == q) break;
        long b = a;
        if (*end == '-') { q = end + 1; b = strtol(q, &end, 10); }
        for (long k = a; k <= b && k < CPU_SETSIZE; k++) CPU_SET((int)k, &want);
        q = (*end == ',') ? end + 1 : end;
        if (*end != ',') break;
    }
    if (sched_getaffinity(0, sizeof(have), &have) != 0) return 0;
    CPU_AND(&both, &want, &have);
    // fewer than 8 CPUs in common (a launcher that pinned this rank elsewhere, a cgroup that grants a sliver of the node): leave the
    // affinity alone -- the rank's main thread spins on the scalar mailbox, and the staging helpers, the file readers and RCCL's
    // proxy threads need cores of their own beside it
    if (CPU_COUNT(&both) < 8) return 0;
    if (sched_setaffinity(0, sizeof(both), &both) != 0) return 0;
    if (numa_node_out) *numa_node_out = node;
    return 0;
}
int gv_ingest_info2(gv_ctx* c, gv_ingest_stats* out) {
    NEED(c, out != nullptr, "gv_ingest_info2: out is NULL");
    out->alloc_seconds = c->ingest_alloc_s;
    out->fill_seconds = c->ingest_fill_s;
    out->overlap_seconds = c->ingest_overlap_s;
    out->resident_bytes = (double)c->ingest_bytes;
    out->layout = gv_get_layout(c);
    out->expected_passes = c->expected_passes;
    return 0;
}
int gv_set_expected_passes(gv_ctx* c, int64_t passes) {
    NEED(c, passes >= 0, "gv_set_expected_passes: passes >= 0 (0 = unknown)");
    c->expected_passes = passes;
    return 0;
}

}  // extern "C"
