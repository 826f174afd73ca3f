// gv_stats.hip -- statistics over the resident dataset: the phenotype mask, marker and people statistics, and the per-marker
// p-values of data::pvals_calc / pvals_calc_LOCO (gv_pvals_*) with the whole test result beside them (gv_assoc_*).
#include <cmath>
#include <cstring>

#include "gv_internal.h"

using namespace gvi;

extern "C" {

int gv_set_mask(gv_ctx* c, const uint8_t* mask4, int64_t nonas) {
    NEED(c, c->N > 0, "gv_set_mask: gv_set_dims must be called first");
    const int64_t P4 = c->pitch / 4;
    std::vector<uint32_t> m2(P4, 0u);
    for (int64_t n = 0; n < c->N; n++) {
        bool present = mask4 ? ((mask4[n >> 2] >> (n & 3)) & 1u) : true;
        if (present) m2[n >> 4] |= 3u << (2 * (n & 15));
    }
    if (!c->mask2) HIPCHK(c, hipMalloc(&c->mask2, sizeof(uint32_t) * P4));
    HIPCHK(c, hipMemcpyAsync(c->mask2, m2.data(), sizeof(uint32_t) * P4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->nonas = nonas;
    c->have_stats = c->have_people = false;
    cov_drop(c);
    pc_invalidate(c, false);
    return 0;
}

int gv_marker_stats(gv_ctx* c, double alpha_scale) {
    pc_invalidate(c, false);
    c->have_people = false;       // (the people statistics are sums over the standardised genotypes: new mave / msig, new sums)
    cov_drop(c);                  // (and so are the covariate side's products)
    if (c->dense.resident) {      // the meth branch of compute_markers_statistics (data.cpp:487-540)
        NEED(c, c->mask2, "gv_marker_stats: mask must be set first");
        gvd::stats(c->stream, dense_view(c), c->mask2, (double)c->nonas, alpha_scale, c->mave);      // (codes: the same, in code units)
        c->alpha_scale = alpha_scale;
        KCHK(c);
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->have_stats = true;
        return 0;
    }
    NEED(c, (c->have_raw || c->have_stripes) && c->mask2, "gv_marker_stats: bed and mask must be set first");
    if (c->have_stripes && c->plan.layout == 1 && (c->kernel_mode != 0 || !c->have_raw))
        gvm::stats_from_tiles(c->stream, c->plan.tiles, c->mask2, c->M, c->plan.nrg_m, c->plan.nkb_m, c->pitch / 4,
                              (double)c->nonas, alpha_scale, c->mave, c->msig, c->counts);
    else if (c->have_stripes && (c->kernel_mode != 0 || !c->have_raw))
        gvm::stats_from_stripes(c->stream, c->plan.stripes_m, c->mask2, c->M, c->plan.nkb_m, c->pitch / 4,
                                (double)c->nonas, alpha_scale, c->mave, c->msig, c->counts);
    else
        gvk::marker_stats(c->stream, c->bed, c->mask2, c->M, c->pitch, (double)c->nonas, alpha_scale, c->mave, c->msig,
                          c->counts);
    c->alpha_scale = alpha_scale;
    KCHK(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->have_stats = true;
    return 0;
}

// the per-marker counts sum b na: what the missing-aware statistics left, nonas for every marker where no entry can be missing
int gv_marker_counts(gv_ctx* c, double* cnt) {
    NEED(c, cnt != nullptr, "gv_marker_counts: cnt is NULL");
    NEED(c, c->dense.resident && c->dense.bits, "gv_marker_counts: the resident dataset is not compact dosage data");
    NEED(c, c->have_stats, "gv_marker_counts: gv_marker_stats has not run");
    if (dosage_na_kernels(c)) {
        HIPCHK(c, hipMemcpyAsync(cnt, c->dense.cnt, sizeof(double) * c->M, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    } else
        for (int64_t m = 0; m < c->M; m++) cnt[m] = (double)c->nonas;
    return 0;
}

int gv_get_marker_stats(gv_ctx* c, double* mave, double* msig) {
    NEED(c, c->have_stats, "gv_get_marker_stats: gv_marker_stats has not run");
    HIPCHK(c, hipMemcpyAsync(mave, c->mave, sizeof(double) * c->M, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(msig, c->msig, sizeof(double) * c->M, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- --use-XXT-denoiser 1: LMMSE through CG in N-space (denoiserXXT.cpp), matrix-free ------------------------------
// data::compute_people_statistics (data.cpp:558-716): three table passes of the fp64 Ax kernel over the raw rows.
int gv_people_stats(gv_ctx* c, double* mave_people, double* msig_people, double* numb_people) {
    REFUSE_DOSAGE(c, "gv_people_stats", "the dense kinds have no people statistics");
    NEED(c, !c->dense.resident, "gv_people_stats: not available for methylation data (the reference's meth branch of "
                            "compute_people_statistics, data.cpp:633-672, never reduces or finalises its sums)");
    NEED(c, c->have_stats && c->mask2, "gv_people_stats: marker statistics must be computed first");
    const bool from_stripes = c->have_stripes && (c->kernel_mode != 0 || !c->have_raw);
    NEED(c, c->have_raw || from_stripes, "gv_people_stats: no genotype layout resident");
    if (ensure_work(c)) return 1;
    for (gv_vec** v : {&c->mave_p, &c->msig_p, &c->numb_p})
        if (!*v && vec_new(c, GV_SPACE_N, v)) return 1;
    gv_vec* dst[3] = {c->mave_p, c->numb_p, c->msig_p};   // kinds 0 (sum value), 1 (count), 2 (sum value^2)
    if (from_stripes) {
        // four passes over stripes_n in exact fixed point: the sum is an Ax of the all-ones vector, the count and the
        // two halves of the sum of squares have their own operand tables (k_prep_people); the quadratic half reads the
        // a^2 plane of the codes (MODE 4 of the streaming kernel)
        hipStream_t s = c->stream;
        if (c->M == 0) {      // an empty shard adds zeros to the three sums, through the same collectives as its peers
            for (int kind = 0; kind < 3; kind++) gvk::fill(s, dst[kind]->d, c->npad, 0.0);
        } else {
            double* ones = c->cg_d->d;
            gvk::fill(s, ones, c->M, 1.0);
            gvm::ax(s, c->plan, ones, c->mave, c->msig, c->mask2, c->npad, 1.0, c->red_partial, c->mave_p->d);
            gvm::ax_people(s, c->plan, 0, c->mave, c->msig, c->mask2, c->npad, c->red_partial, c->numb_p->d);
            gvm::ax_people(s, c->plan, 1, c->mave, c->msig, c->mask2, c->npad, c->red_partial, c->msig_p->d);
            gvm::ax_people(s, c->plan, 2, c->mave, c->msig, c->mask2, c->npad, c->red_partial, c->w_n->d);
            gvk::axpby(s, c->msig_p->d, 1.0, c->msig_p->d, 1.0, c->w_n->d, c->npad);
        }
        KCHK(c);
        for (int kind = 0; kind < 3; kind++)
            if (comm_allreduce(c, dst[kind]->d, c->npad)) return 1;     // data.cpp:604-606
    }
    for (int kind = 0; kind < 3 && !from_stripes; kind++) {
        gvk::people_table(c->stream, c->mave, c->msig, c->M, kind, c->t3);
        gvk::ax_f64(c->stream, c->bed, c->M, c->pitch, c->t3, c->ax_chunks, c->ax_partial, c->npad);
        gvk::ax_reduce(c->stream, c->ax_partial, c->ax_chunks, c->npad, c->mask2, 1.0, dst[kind]->d);
        KCHK(c);
        if (comm_allreduce(c, dst[kind]->d, c->npad)) return 1;     // data.cpp:604-606
    }
    gvk::people_finish(c->stream, c->mave_p->d, c->msig_p->d, c->numb_p->d, c->mask2, c->N, c->npad);
    KCHK(c);
    const size_t n4 = sizeof(double) * 4 * c->mbytes;
    if (mave_people) HIPCHK(c, hipMemcpyAsync(mave_people, c->mave_p->d, n4, hipMemcpyDeviceToHost, c->stream));
    if (msig_people) HIPCHK(c, hipMemcpyAsync(msig_people, c->msig_p->d, n4, hipMemcpyDeviceToHost, c->stream));
    if (numb_people) HIPCHK(c, hipMemcpyAsync(numb_people, c->numb_p->d, n4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->have_people = true;
    return 0;
}

// ---- p-values: data::pvals_calc (data.cpp:1108-1226) and pvals_calc_LOCO (:1235-1353), one estimator ----------------
// Kernel mode 1: per call ONE pass over the shard whose epilogue runs the per-marker regression test (gvm::marker_pvals: operands,
// digits, stream, test -- four launches, no allocation: the operands live in the context's N-space scratch, the p-values in an
// M-space work vector until they are copied out).  Kernel mode 0 (fp64 family, parity anchor): the sums of k_marker_sums2_f64, then
// the stand-alone test kernel.
// out4[4m..] = {sum a p, sum b p, sum a p^2, sum b p^2} for the N-space device vector p, fp64 family
static int marker_sums_p_p2_f64(gv_ctx* c, const double* p, double* p2_scratch, double* out4_dev) {
    NEED(c, c->have_raw, "p-values: kernel mode 0 needs the raw row layout");
    gvk::mul(c->stream, p2_scratch, p, p, c->npad);
    gvk::marker_sums2_f64(c->stream, c->bed, c->M, c->pitch, p, p2_scratch, out4_dev);
    KCHK(c);
    return 0;
}

// chrom == NULL: leave-one-out (the marker's own effect is added back analytically); else leave-one-chromosome-out.
// One loop for both entry-point families.  out[0] = p-values; assoc (gv_assoc_*): out[1..3] = beta, se, t as well (host pointers, each
// may be NULL), compact dense data take the marker pass of their own (gvd::assoc) and the bed families the passes of gv_pvals_*
// with the wide epilogue.  assoc == false is gv_pvals_* to the bit: the narrow epilogue kernels, the same launches in the same order.
static int pvals_impl(gv_ctx* c, bool assoc, const gv_vec* z1, const gv_vec* y, const gv_vec* x1_hat, const int* chrom,
                      double* const (&out)[4], double* chrom_pred = nullptr) {
    const char* who = assoc ? "gv_assoc" : "gv_pvals";
    if (assoc)
        NEED(c, !(c->dense.resident && !c->dense.bits), "gv_assoc: not available for methylation data (dense fp64 matrix): the reference's "
                                                    "meth branch of pvals_calc, data.cpp:1187-1223, defines no test and none is defined here");
    else {
        REFUSE_DOSAGE(c, "gv_pvals", "the dense kinds compute no p-values");
        NEED(c, !c->dense.resident, "gv_pvals: not available for methylation data (the reference's meth branch of pvals_calc, "
                                "data.cpp:1187-1223, computes and stores nothing)");
    }
    if (!(z1->space == GV_SPACE_N && y->space == GV_SPACE_N && x1_hat->space == GV_SPACE_M)) return fail(c, "%s: bad vector spaces", who);
    NEED_VEC(c, who, z1, GV_SPACE_N);
    NEED_VEC(c, who, y, GV_SPACE_N);
    NEED_VEC(c, who, x1_hat, GV_SPACE_M);
    if (!c->have_stats) return fail(c, "%s: marker statistics must be computed first", who);
    if (ensure_work(c) || ensure_w2(c)) return 1;
    const int64_t M = c->M;
    const double sqrtN = sqrt((double)c->N);
    const bool dosage = c->dense.resident;            // (assoc only: gv_pvals_* has refused the dense kinds above)
    const bool fused = !dosage && c->kernel_mode != 0;      // (kernel mode 2: the p-value pass is mode 1's -- its sums run over exact planes already)
    if (fused && M > 0) {
        NEED(c, c->have_stripes, "p-values: kernel modes 1 and 2 need a re-encoded layout");
        if (!c->ks_tuned && autotune_ks(c)) return 1;      // (a p-value call may be the first streaming pass of a context)
    }
    gv_vec *ymod = nullptr, *ych = nullptr, *sq = nullptr, *xch = nullptr, *wide[3] = {nullptr, nullptr, nullptr};
    double* sums_dev = nullptr;
    int* chrom_dev = nullptr;
    int64_t* rows_dev = nullptr;
    int rc = 0;
    const size_t Mn = (size_t)(M > 0 ? M : 1);
    auto cleanup = [&]() {
        for (gv_vec* v : {ymod, ych, sq, xch, wide[0], wide[1], wide[2]}) vec_del(c, v);
        if (sums_dev) (void)hipFree(sums_dev);
        if (chrom_dev) (void)hipFree(chrom_dev);
        if (rows_dev) (void)hipFree(rows_dev);
    };
#define PV_TRY(expr) do { if ((rc = (expr)) != 0) { cleanup(); return rc; } } while (0)
#define PV_HIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { cleanup(); return fail(c, "%s failed: %s", #expr, hipGetErrorString(e_)); } } while (0)
    // an M-space work vector of the CG: INVARIANT -- ax_device / ax_overlapped (run per chromosome between the marker passes of the LOCO
    // loop below) never touch the CG work vectors cg_r / cg_z / cg_p / cg_d; gv_ax / gv_atx (which stage through cg_d) are host entry
    // points and cannot run inside this call
    double* pv_dev = c->cg_d->d;
    double *pa = c->w_n->d, *pb = c->w_n2->d;   // operands of the fused pass: p and p^2 (compact dense data: pa holds the residual)
    gvm::PvArgs pva{c->counts, nullptr, 0.0, nullptr, 0};
    if (assoc) {
        for (int k = 0; k < 3; k++) PV_TRY(vec_new(c, GV_SPACE_M, &wide[k]));
        pva.beta = wide[0]->d; pva.se = wide[1]->d; pva.t = wide[2]->d;
    }
    if (!fused && !dosage) {
        PV_TRY(vec_new(c, GV_SPACE_N, &ymod));
        PV_TRY(vec_new(c, GV_SPACE_N, &sq));
        PV_HIP(hipMalloc(&sums_dev, sizeof(double) * 4 * Mn));
        gvk::axpby(c->stream, ymod->d, 1.0, y->d, -1.0, z1->d, c->npad);            // y_mod = y - z1 (data.cpp:1117-1119)
        // the reference masks every term of the regression sums with na_lut[mask4] (data.cpp:1155-1175); the sums here are
        // matvec-shaped and need zeros at NA / pad slots instead, whatever the caller left there (an unfiltered y holds DBL_MAX)
        gvk::mask_copy(c->stream, ymod->d, ymod->d, c->mask2, c->npad);
    }
    // the marker pass of one residual: add == NULL, every marker with its own effect added back (leave-one-out); else the markers of
    // chromosome ch -- compact dense data: the rows rows_dev[r0 .. r0 + nr) -- against y - z1 + add
    auto marker_pass = [&](double* add, int ch, int64_t r0, int64_t nr) -> int {
        if (M == 0) return 0;      // (an empty shard has no marker to test)
        const bool loo = add == nullptr;
        if (dosage) {
            gvd::assoc_prep(c->stream, y->d, z1->d, add, c->mask2, c->npad, pa, c->red_partial, c->red_out);
            gvd::assoc(c->stream, dense_view(c), loo ? nullptr : rows_dev + r0, loo ? M : nr, pa, c->mask2, c->red_out, (double)c->nonas,
                       loo ? x1_hat->d : nullptr, 1.0 / sqrtN, pva.beta, pva.se, pva.t, pv_dev);
        } else if (fused) {
            pva.xself = loo ? x1_hat->d : nullptr;      // y_mark = y_mod + gen_part * x1_hat[k] (data.cpp:1145-1148): c = x1_hat[k] / sqrt(N)
            pva.self_scale = loo ? 1.0 / sqrtN : 0.0;
            pva.chrom = loo ? nullptr : chrom_dev;
            pva.ch = ch;
            gvm::marker_pvals(c->stream, c->plan, y->d, z1->d, add, c->mask2, c->npad, c->mave, c->msig, pa, pb, c->red_partial, pva, pv_dev);
        } else {
            if (!loo) gvk::axpby(c->stream, add, 1.0, add, 1.0, ymod->d, c->npad);   // p = chromosome predictor + y_mod (:1284)
            if (marker_sums_p_p2_f64(c, loo ? ymod->d : add, sq->d, sums_dev)) return 1;
            gvk::pvals_test(c->stream, c->counts, c->mave, c->msig, sums_dev, loo ? x1_hat->d : nullptr, loo ? 1.0 / sqrtN : 0.0,
                            loo ? nullptr : chrom_dev, ch, M, pv_dev, pva.beta, pva.se, pva.t);
        }
        return 0;
    };
    if (!chrom) {
        PV_TRY(marker_pass(nullptr, 0, 0, M));
    } else {
        PV_HIP(hipMemsetAsync(pv_dev, 0, sizeof(double) * Mn, c->stream));      // markers of chromosomes outside 1..23 keep 0
        for (gv_vec* v : wide)
            if (v) PV_HIP(hipMemsetAsync(v->d, 0, sizeof(double) * Mn, c->stream));
        PV_TRY(vec_new(c, GV_SPACE_N, &ych));
        PV_TRY(vec_new(c, GV_SPACE_M, &xch));
        PV_HIP(hipMalloc(&chrom_dev, sizeof(int) * Mn));
        PV_HIP(hipMemcpyAsync(chrom_dev, chrom, sizeof(int) * M, hipMemcpyHostToDevice, c->stream));
        double present[24];
        for (int ch = 0; ch < 24; ch++) present[ch] = 0;
        for (int64_t k = 0; k < M; k++) if (chrom[k] >= 1 && chrom[k] <= 23) present[chrom[k]] += 1;
        // compact dense data: the rows of every chromosome side by side, in marker order, so that the pass for chromosome ch streams
        // that chromosome's rows alone -- the 23 passes together read the matrix once
        int64_t row0[25] = {0};
        std::vector<int64_t> rows_host;
        if (dosage) {
            for (int ch = 1; ch <= 23; ch++) row0[ch + 1] = row0[ch] + (int64_t)present[ch];
            rows_host.resize(Mn);
            int64_t fill[24];
            for (int ch = 1; ch <= 23; ch++) fill[ch] = row0[ch];
            for (int64_t k = 0; k < M; k++) if (chrom[k] >= 1 && chrom[k] <= 23) rows_host[fill[chrom[k]]++] = k;
            PV_HIP(hipMalloc(&rows_dev, sizeof(int64_t) * Mn));
            PV_HIP(hipMemcpyAsync(rows_dev, rows_host.data(), sizeof(int64_t) * Mn, hipMemcpyHostToDevice, c->stream));
            PV_HIP(hipStreamSynchronize(c->stream));      // (rows_host is pageable memory of this frame)
        }
        PV_TRY(allreduce_scalars(c, present, 24));
        if (chrom_pred) memset(chrom_pred, 0, sizeof(double) * 23 * 4 * (size_t)c->mbytes);   // chromosomes nobody holds: zeros
        for (int ch = 1; ch <= 23; ch++) {
            if (present[ch] == 0) continue;      // no rank holds a marker of this chromosome
            gvk::select_eq(c->stream, xch->d, x1_hat->d, chrom_dev, ch, M);
            PV_TRY(ax_device(c, xch->d, ych->d));                                // chromosome predictor, all ranks (:1268-1272)
            if (chrom_pred)                                                      // the vector the reference dumps (:1276-1281)
                PV_TRY(to_host(c, chrom_pred + (size_t)(ch - 1) * 4 * c->mbytes, ych->d, sizeof(double) * 4 * c->mbytes));
            PV_TRY(marker_pass(ych->d, ch, row0[ch], row0[ch + 1] - row0[ch]));
        }
    }
    KCHK(c);
    if (M > 0) {
        double* const dev[4] = {pv_dev, pva.beta, pva.se, pva.t};
        for (int k = 0; k < 4; k++)
            if (out[k] && dev[k]) PV_TRY(to_host(c, out[k], dev[k], sizeof(double) * M));
    }
#undef PV_TRY
#undef PV_HIP
    if (ymod || ych || sq || xch || wide[0] || sums_dev || chrom_dev || rows_dev) HIPCHK(c, hipStreamSynchronize(c->stream));
    cleanup();
    return 0;
}

int gv_pvals_loo(gv_ctx* c, const gv_vec* z1, const gv_vec* y, const gv_vec* x1_hat, double* pvals) {
    return pvals_impl(c, false, z1, y, x1_hat, nullptr, {pvals, nullptr, nullptr, nullptr});
}
int gv_pvals_loco(gv_ctx* c, const gv_vec* z1, const gv_vec* y, const gv_vec* x1_hat, const int* chrom, double* pvals) {
    NEED(c, chrom != nullptr, "gv_pvals_loco: chrom is NULL");
    return pvals_impl(c, false, z1, y, x1_hat, chrom, {pvals, nullptr, nullptr, nullptr});
}
int gv_pvals_loco_pred(gv_ctx* c, const gv_vec* z1, const gv_vec* y, const gv_vec* x1_hat, const int* chrom, double* pvals,
                       double* chrom_pred) {
    NEED(c, chrom != nullptr, "gv_pvals_loco_pred: chrom is NULL");
    return pvals_impl(c, false, z1, y, x1_hat, chrom, {pvals, nullptr, nullptr, nullptr}, chrom_pred);
}

// the whole test result: p through the passes of gv_pvals_* (bed data) or the pass of compact dense data, beta / se / t beside it
int gv_assoc_loo(gv_ctx* c, const gv_vec* z1, const gv_vec* y, const gv_vec* x1_hat, const gv_assoc_out* out) {
    NEED(c, out != nullptr, "gv_assoc_loo: out is NULL");
    return pvals_impl(c, true, z1, y, x1_hat, nullptr, {out->p, out->beta, out->se, out->t});
}
int gv_assoc_loco(gv_ctx* c, const gv_vec* z1, const gv_vec* y, const gv_vec* x1_hat, const int* chrom, const gv_assoc_out* out,
                  double* chrom_pred) {
    NEED(c, out != nullptr, "gv_assoc_loco: out is NULL");
    NEED(c, chrom != nullptr, "gv_assoc_loco: chrom is NULL");
    return pvals_impl(c, true, z1, y, x1_hat, chrom, {out->p, out->beta, out->se, out->t}, chrom_pred);
}

}  // extern "C"
