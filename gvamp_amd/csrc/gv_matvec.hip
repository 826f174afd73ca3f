// gv_matvec.hip -- data::Ax / data::ATx of the C ABI: one dispatcher per product direction (ax_pass / atx_pass) over the launchers
// of the dense kinds (gvd::ax_partial / ax_reduce / atx on the context's DenseData, whatever its width: fp64 methylation data, 8- /
// 16-bit dosage codes) and the three genotype kernel families, the N-space exchange of a sharded job (in one piece, or overlapped
// with the decode), and the event pairs of set_timing 2.
#include <cmath>

#include "gv_internal.h"

namespace gvi {

// timing == 2: resolve the pending event pairs into the kernel counters
void ev_resolve(gv_ctx* c) {
    for (size_t i = 0; i < c->ev_used; i++) {
        gv_ctx::EvRec& r = c->ev_pool[i];
        float ms = 0;
        if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            if (r.kind == 0) { c->cnt.ms_ax_kernel += ms; c->cnt.n_ax_kernel++; }
            else if (r.kind == 1) { c->cnt.ms_atx_kernel += ms; c->cnt.n_atx_kernel++; }
            else { c->cnt.ms_allreduce += ms; c->cnt.n_allreduce++; }
        }
    }
    c->ev_used = 0;
}
static gv_ctx::EvRec* ev_next(gv_ctx* c, int kind) {
    if (c->timing != 2) return nullptr;
    if (c->ev_used == 4096) ev_resolve(c);
    if (c->ev_used == c->ev_pool.size()) {
        gv_ctx::EvRec r{nullptr, nullptr, kind};
        if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) return nullptr;
        c->ev_pool.push_back(r);
    }
    gv_ctx::EvRec* r = &c->ev_pool[c->ev_used++];
    r->kind = kind;
    return r;
}

// ---- the exchange step of data::Ax (data.cpp:928/:995) overlapped with the decode (north_star; GV_OVERLAP=T or gv_set_overlap)
// The product is cut into T chunks of individuals (whole quads of row groups).  Chunk t is decoded on the context's stream;
// its slice of the N-vector is all-reduced and scaled on a side stream while chunk t + 1 decodes; the context's stream joins
// the side stream at the end.  Every chunk is the same exact integer arithmetic as the undivided pass and the all-reduce
// of a slice adds the same numbers in the same rank order: results are bit-identical to the one-message form.  What it
// buys is (T - 1)/T of the exchange time at the price of T - 1 more kernel tails (docs/history/rounds1-3.md section 6): a knob to measure
// on an 8-GPU node, off by default.
int ax_overlapped(gv_ctx* c, int nv, const double* xa, const double* xb, double* outa, double* outb,
                  const gvm::CgHook* cg) {
    const double scale = 1.0 / sqrt((double)c->N);
    gvm::Plan& pl = c->plan;
    if (!c->comm_stream) {
        HIPCHK(c, hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_chunk, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_comm, hipEventDisableTiming));
    }
    // The slices are cut from N alone, in units of 1024 individuals -- a whole number of row-group quads in either resident
    // layout (4 x 4 x 64 rows on two stripe sets, 4 x 256 rows on the tile layout): the ranks of one job may hold different
    // layouts (gv_set_layout(.., 3) decides per rank from its free HBM) and must still exchange the same ranges.
    const int64_t nu = (c->N + 1023) / 1024;
    int T = c->overlap_tiles;
    if (T > nu) T = (int)nu;
    const int64_t gpu_ = 1024 / pl.rows_n;      // row groups per unit: 16 or 4
    const bool empty = c->M == 0;      // an empty shard sends zeros through the same sequence of slice messages
    if (empty) {
        gvk::fill(c->stream, outa, c->npad, 0.0);
        if (nv == 2) gvk::fill(c->stream, outb, c->npad, 0.0);
    } else
        gvm::ax_prep(c->stream, pl, xa, nv == 2 ? xb : nullptr, c->mave, c->msig, c->red_partial, cg);
    for (int t = 0; t < T; t++) {
        const int64_t u0 = nu * t / T, u1 = nu * (t + 1) / T;
        int64_t rg0 = u0 * gpu_, rg1 = t == T - 1 ? pl.nrg_n : u1 * gpu_;
        if (rg0 > pl.nrg_n) rg0 = pl.nrg_n;
        if (rg1 > pl.nrg_n) rg1 = pl.nrg_n;
        if (!empty && rg1 > rg0) gvm::ax_rows(c->stream, pl, nv, rg0, rg1, c->mask2, c->npad, 1.0, outa, nv == 2 ? outb : nullptr, cg);
        KCHK(c);
        const int64_t n0 = u0 * 1024;
        const int64_t cnt = (t == T - 1 ? c->npad : u1 * 1024) - n0;    // the last slice takes the pad tail (zeros) along
        if (cnt <= 0) continue;
        HIPCHK(c, hipEventRecord(c->ev_chunk, c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->comm_stream, c->ev_chunk, 0));
        if (comm_allreduce_on(c, outa + n0, (size_t)cnt, c->comm_stream)) return 1;
        gvk::scale_vec(c->comm_stream, outa + n0, cnt, scale);
        if (nv == 2) {
            if (comm_allreduce_on(c, outb + n0, (size_t)cnt, c->comm_stream)) return 1;
            gvk::scale_vec(c->comm_stream, outb + n0, cnt, scale);
        }
        KCHK(c);
    }
    HIPCHK(c, hipEventRecord(c->ev_comm, c->comm_stream));
    if (!(c->force_multi & 4))     // (bit 4 of gv_debug_force_multi: fault injection for tests/test_gpu_forced_multi.py -- the join is dropped)
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_comm, 0));
    return 0;
}
bool use_overlap(const gv_ctx* c) {   // nothing rank-local in here (have_stripes: every rank holds SOME re-encoded layout, whichever)
    return c->overlap_tiles > 1 && is_multi(c) && c->kernel_mode == 1 && c->have_stripes;
}

// ---- the exchange step of a pass on a multi-rank context: data.cpp:995 / :1034 MPI_Allreduce, then the 1/sqrt(N) of :998-1005 /
// :1036-1037 (pad slots stay exact zeros).  One message and one scaling pass when the outputs are the context's own w_n | w_n2
// (one allocation), otherwise nv messages followed by nv scalings.  Shared by the dense and the genotype products.
static int exchange_n(gv_ctx* c, int nv, double* outa, double* outb) {
    const double scale = 1.0 / sqrt((double)c->N);
    Timer t(c, &c->cnt.ms_allreduce);
    gv_ctx::EvRec* er = ev_next(c, 2);                 // timing == 2: the exchange step of the pass, un-synchronised
    if (er) (void)hipEventRecord(er->a, c->stream);
    if (nv == 2 && c->w_n && c->w_n2 && outa == c->w_n->d && outb == c->w_n2->d) {
        if (comm_allreduce(c, outa, 2 * c->npad)) return 1;
        gvk::scale_vec(c->stream, outa, 2 * c->npad, scale);
    } else {
        if (comm_allreduce(c, outa, c->npad)) return 1;
        if (nv == 2 && comm_allreduce(c, outb, c->npad)) return 1;
        gvk::scale_vec(c->stream, outa, c->npad, scale);
        if (nv == 2) gvk::scale_vec(c->stream, outb, c->npad, scale);
    }
    if (er) (void)hipEventRecord(er->b, c->stream);
    KCHK(c);
    t.stop();
    if (c->timing == 1) c->cnt.n_allreduce++;
    return 0;
}

// data::Ax on device pointers, nv = 1 or 2 vectors.  x: M doubles, out: npad doubles.  ONE pass over the shard on methylation
// data (gv_dense.hip: dispatched ahead of the kernel mode and the layout) and in kernel mode 1; in kernel modes 0 and 2 two
// vectors are two complete single passes.
// The collective sequence must not depend on rank-local state (an empty shard, M == 0, enters the same calls with zeros): it
// is chosen by the kind of data, the kernel mode, use_overlap -- the same on every rank of a job -- and the output pointers only.
int ax_pass(gv_ctx* c, int nv, const double* xa, const double* xb, double* outa, double* outb, const gvm::CgHook* cg) {
    const bool dense = c->dense.resident;
    // (the hooks of the device-resident loops exist in gvm::ax / ax2 / ax_rows only: cgx_usable keeps every caller to kernel mode 1)
    NEED(c, !cg || (!dense && c->kernel_mode == 1), dense ? "Ax: the device-resident CG does not run on methylation data"
                                                          : "Ax: the device-resident CG runs in kernel mode 1 only");
    if (nv == 2 && !dense && c->kernel_mode != 1) {
        if (ax_pass(c, 1, xa, nullptr, outa, nullptr, nullptr)) return 1;
        return ax_pass(c, 1, xb, nullptr, outb, nullptr, nullptr);
    }
    NEED(c, c->have_stats && c->mask2, dense ? "Ax: methylation data, mask and marker statistics must be set first"
                                             : "Ax: bed, mask and marker statistics must be set first");
    const double scale = 1.0 / sqrt((double)c->N);
    const bool multi = is_multi(c);
    const bool overlap = !dense && use_overlap(c);
    if (overlap) {
        if (c->M > 0 && !c->ks_tuned && autotune_ks(c)) return 1;
        c->plan.ev0 = c->plan.ev1 = nullptr;
        if (ax_overlapped(c, nv, xa, xb, outa, outb, cg)) return 1;
    } else if (c->M == 0) {   // an empty shard (Mt < ranks) contributes zeros through the same collective as its peers
        gvk::fill(c->stream, outa, c->npad, 0.0);
        if (nv == 2) gvk::fill(c->stream, outb, c->npad, 0.0);
        KCHK(c);
    } else {
        const bool mfma = !dense && c->kernel_mode != 0;
        gvd::AxShape sh;
        const bool fixed = dense && dosage_mfma_route(c);      // 8-bit codes on the fixed-point route (gv_set_dosage_route)
        if (fixed)
            HIPCHK(c, gvdm::reserve(c->dense.fx, c->N, c->M, c->dense.cus, c->dosage_seg));
        else if (dense) {
            DenseData& d = c->dense;
            sh = gvd::ax_shape(c->N, c->M, d.cus, gvd::ax_cols(d.bits));
            const size_t need = (size_t)2 * sh.segs * c->npad;
            if (need > d.part_cap) {
                if (d.part) (void)hipFree(d.part);
                d.part = nullptr;
                d.part_cap = 0;
                HIPCHK(c, hipMalloc(&d.part, sizeof(double) * need));
                d.part_cap = need;
            }
        } else if (mfma) {
            NEED(c, c->have_stripes, nv == 2 ? "Ax: kernel mode 1 needs the stripe layouts (gv_set_layout before ingest)"
                                             : "Ax: kernel modes 1 and 2 need a re-encoded layout (gv_set_layout before ingest)");
            if (!c->ks_tuned && autotune_ks(c)) return 1;
        } else
            NEED(c, c->have_raw, "Ax: kernel mode 0 needs the raw row layout (not the default: gv_set_layout(ctx, 1, ..) before ingest)");
        Timer t(c, &c->cnt.ms_ax);
        gv_ctx::EvRec* er = ev_next(c, 0);     // timing == 2: around the streaming kernel (the MFMA family records the pair itself)
        if (fixed)
            gvdm::ax(c->stream, nv, dense_view(c), c->dense.fx, gvdm::ax_shape(c->N, c->M, c->dense.cus, c->dosage_seg), xa, nv == 2 ? xb : xa,
                     c->npad, multi ? 1.0 : scale, outa, nv == 2 ? outb : outa, er ? er->a : nullptr, er ? er->b : nullptr);
        else if (dense) {
            if (er) (void)hipEventRecord(er->a, c->stream);
            gvd::ax_partial(c->stream, nv, sh, dense_view(c), xa, nv == 2 ? xb : xa, c->dense.part, c->npad);
            if (er) (void)hipEventRecord(er->b, c->stream);
            gvd::ax_reduce(c->stream, nv, sh, c->dense.part, c->N, c->npad, multi ? 1.0 : scale, outa, nv == 2 ? outb : outa);
        } else if (mfma) {
            c->plan.ev0 = er ? er->a : nullptr;
            c->plan.ev1 = er ? er->b : nullptr;
            if (nv == 2)
                gvm::ax2(c->stream, c->plan, xa, xb, c->mave, c->msig, c->mask2, c->npad, multi ? 1.0 : scale, c->red_partial, outa, outb, cg);
            else if (c->kernel_mode == 2)      // two-level fixed point: head and residual of x in the two slots of one pass (no CG hooks in this mode)
                gvm::ax_wide(c->stream, c->plan, xa, c->mave, c->msig, c->mask2, c->npad, multi ? 1.0 : scale, c->red_partial, outa);
            else
                gvm::ax(c->stream, c->plan, xa, c->mave, c->msig, c->mask2, c->npad, multi ? 1.0 : scale, c->red_partial, outa, cg);
        } else {
            gvk::ax_table(c->stream, xa, c->mave, c->msig, c->M, c->t3);
            if (er) (void)hipEventRecord(er->a, c->stream);
            gvk::ax_f64(c->stream, c->bed, c->M, c->pitch, c->t3, c->ax_chunks, c->ax_partial, c->npad);
            if (er) (void)hipEventRecord(er->b, c->stream);
            gvk::ax_reduce(c->stream, c->ax_partial, c->ax_chunks, c->npad, c->mask2, multi ? 1.0 : scale, outa);
        }
        KCHK(c);
        t.stop();
    }
    c->cnt.n_ax += nv;
    c->cnt.n_ax_pass += 1;
    if (multi && !overlap) return exchange_n(c, nv, outa, outb);      // (the overlapped path has exchanged its slices already)
    return 0;
}

// data::ATx on device pointers, nv = 1 or 2 vectors.  p: npad doubles (zero at NA / pad slots), out: M doubles; then
// out = tau * out + gam2 * addx when addx != NULL.  ONE pass on methylation data and in kernel mode 1 on a re-encoded layout, two
// complete single passes otherwise.  No collective in ATx.
int atx_pass(gv_ctx* c, int nv, const double* pa, const double* pb, double* outa, double* outb, const double* addxa,
             const double* addxb, double tau, double gam2, const gvm::CgHook* cg) {
    const bool dense = c->dense.resident;
    NEED(c, !cg || (!dense && c->kernel_mode == 1), dense ? "ATx: the device-resident CG does not run on methylation data"
                                                          : "ATx: the device-resident CG runs in kernel mode 1 only");
    // (the two-vector form of an empty genotype shard has never asked for the statistics it does not read)
    NEED(c, c->have_stats || (!dense && nv == 2 && c->M == 0), dense ? "ATx: methylation data and marker statistics must be set first"
                                                                      : "ATx: bed and marker statistics must be set first");
    if (c->M == 0) {   // empty shard: no markers; the <d,p> a CG hook asks for is 0 from this rank (it is all-reduced next)
        for (int k = 0; k < nv && cg; k++) {
            if (cg->dot_out[k]) gvk::fill(c->stream, cg->dot_out[k], 8, 0.0);
            // (the N-space search direction a pass would have advanced on its way in -- CgHook::pn -- is replicated on every rank)
            if (cg->pn[k]) gvk::p_update_st(c->stream, cg->pn[k], cg->zn[k], cg->state[k], c->npad);
        }
        KCHK(c);
    } else if (nv == 2 && !dense && !(c->kernel_mode == 1 && c->have_stripes)) {
        if (atx_pass(c, 1, pa, nullptr, outa, nullptr, addxa, nullptr, tau, gam2, nullptr)) return 1;
        return atx_pass(c, 1, pb, nullptr, outb, nullptr, addxb, nullptr, tau, gam2, nullptr);
    } else {
        const double scale = 1.0 / sqrt((double)c->N);
        const bool mfma = !dense && c->kernel_mode != 0;
        if (mfma) {
            NEED(c, c->have_stripes, "ATx: kernel modes 1 and 2 need a re-encoded layout (gv_set_layout before ingest)");
            if (!c->ks_tuned && autotune_ks(c)) return 1;
        } else if (!dense)
            NEED(c, c->have_raw, "ATx: kernel mode 0 needs the raw row layout (not the default: gv_set_layout(ctx, 1, ..) before ingest)");
        const bool fixed = dense && dosage_mfma_route(c);      // 8-bit codes on the fixed-point route (gv_set_dosage_route)
        if (fixed) HIPCHK(c, gvdm::reserve(c->dense.fx, c->N, c->M, c->dense.cus, c->dosage_seg));
        Timer t(c, &c->cnt.ms_atx);
        gv_ctx::EvRec* er = ev_next(c, 1);
        if (fixed)
            gvdm::atx(c->stream, nv, dense_view(c), c->dense.fx, gvdm::atx_shape(c->N, c->M, c->dense.cus, c->dosage_seg), pa, nv == 2 ? pb : pa,
                      scale, outa, nv == 2 ? outb : outa, addxa, nv == 2 ? addxb : addxa, tau, gam2, er ? er->a : nullptr,
                      er ? er->b : nullptr);
        else if (dense) {
            if (er) (void)hipEventRecord(er->a, c->stream);
            gvd::atx(c->stream, nv, dense_view(c), pa, nv == 2 ? pb : pa, scale, outa, nv == 2 ? outb : outa, addxa, nv == 2 ? addxb : addxa,
                     tau, gam2);
            if (er) (void)hipEventRecord(er->b, c->stream);
        } else if (mfma) {
            c->plan.ev0 = er ? er->a : nullptr;
            c->plan.ev1 = er ? er->b : nullptr;
            if (nv == 2)
                gvm::atx2(c->stream, c->plan, pa, pb, c->npad, c->mave, c->msig, scale, c->red_partial, outa, outb, addxa, addxb, tau, gam2, cg);
            else if (c->kernel_mode == 2)
                gvm::atx_wide(c->stream, c->plan, pa, c->npad, c->mave, c->msig, scale, c->red_partial, outa, addxa, tau, gam2);
            else
                gvm::atx(c->stream, c->plan, pa, c->npad, c->mave, c->msig, scale, c->red_partial, outa, addxa, tau, gam2, cg);
        } else {
            if (er) (void)hipEventRecord(er->a, c->stream);
            gvk::atx_f64(c->stream, c->bed, c->M, c->pitch, pa, c->mave, c->msig, scale, outa);
            if (er) (void)hipEventRecord(er->b, c->stream);
            if (addxa) gvk::axpby(c->stream, outa, tau, outa, gam2, addxa, c->M);
        }
        KCHK(c);
        t.stop();
    }
    c->cnt.n_atx += nv;
    c->cnt.n_atx_pass += 1;
    return 0;
}

int lmmse_device(gv_ctx* c, const double* v, double tau, double gam2, double* out) {
    if (ensure_work(c)) return 1;
    if (ax_device(c, v, c->w_n->d)) return 1;
    return atx_device(c, c->w_n->d, out, v, tau, gam2);   // res = tau * A^T A v + gam2 v (vamp.cpp:1112-1115), in the ATx epilogue
}

}  // namespace gvi

using namespace gvi;

extern "C" {

int gv_ax_dev(gv_ctx* c, const gv_vec* x, gv_vec* out) {
    NEED(c, x->space == GV_SPACE_M && out->space == GV_SPACE_N, "gv_ax_dev: x must be M-space, out N-space");
    NEED_VEC(c, "gv_ax_dev", x, GV_SPACE_M);
    NEED_VEC(c, "gv_ax_dev", out, GV_SPACE_N);
    return ax_device(c, x->d, out->d);
}
int gv_atx_dev(gv_ctx* c, const gv_vec* p, gv_vec* out) {
    NEED(c, p->space == GV_SPACE_N && out->space == GV_SPACE_M, "gv_atx_dev: p must be N-space, out M-space");
    NEED_VEC(c, "gv_atx_dev", p, GV_SPACE_N);
    NEED_VEC(c, "gv_atx_dev", out, GV_SPACE_M);
    return atx_device(c, p->d, out->d);
}

int gv_ax2_dev(gv_ctx* c, const gv_vec* xa, const gv_vec* xb, gv_vec* outa, gv_vec* outb) {
    NEED(c, xa->space == GV_SPACE_M && xb->space == GV_SPACE_M && outa->space == GV_SPACE_N && outb->space == GV_SPACE_N &&
                outa != outb, "gv_ax2_dev: x M-space, out N-space, distinct outputs");
    NEED_VEC(c, "gv_ax2_dev", xa, GV_SPACE_M);
    NEED_VEC(c, "gv_ax2_dev", xb, GV_SPACE_M);
    NEED_VEC(c, "gv_ax2_dev", outa, GV_SPACE_N);
    NEED_VEC(c, "gv_ax2_dev", outb, GV_SPACE_N);
    if (ensure_work(c)) return 1;
    return ax2_device(c, xa->d, xb->d, outa->d, outb->d);
}
int gv_atx2_dev(gv_ctx* c, const gv_vec* pa, const gv_vec* pb, gv_vec* outa, gv_vec* outb) {
    NEED(c, pa->space == GV_SPACE_N && pb->space == GV_SPACE_N && outa->space == GV_SPACE_M && outb->space == GV_SPACE_M &&
                outa != outb, "gv_atx2_dev: p N-space, out M-space, distinct outputs");
    NEED_VEC(c, "gv_atx2_dev", pa, GV_SPACE_N);
    NEED_VEC(c, "gv_atx2_dev", pb, GV_SPACE_N);
    NEED_VEC(c, "gv_atx2_dev", outa, GV_SPACE_M);
    NEED_VEC(c, "gv_atx2_dev", outb, GV_SPACE_M);
    if (ensure_work(c)) return 1;
    return atx2_device(c, pa->d, pb->d, outa->d, outb->d);
}

int gv_ax(gv_ctx* c, const double* x, double* out) {
    if (ensure_work(c)) return 1;
    if (to_device(c, c->cg_d->d, x, sizeof(double) * c->M, false)) return 1;   // the kernels queue up behind the copy
    if (ax_device(c, c->cg_d->d, c->w_n->d)) return 1;
    return to_host(c, out, c->w_n->d, sizeof(double) * 4 * c->mbytes);
}
int gv_atx(gv_ctx* c, const double* p, double* out) {
    if (ensure_work(c)) return 1;
    NEED(c, c->mask2, "gv_atx: the phenotype mask must be set first");
    if (to_device(c, c->w_n->d, p, sizeof(double) * 4 * c->mbytes, false)) return 1;
    // The kernels (like data::dot_product, data.cpp:728-801, which applies no mask) need p = 0 at NA-phenotype and pad
    // slots; the reference's callers hand in filter_pheno()'d vectors.  A caller-owned host vector is not trusted to be
    // filtered -- data::get_phen() carries DBL_MAX at NA individuals (data.cpp:147) -- so the staged copy is masked here:
    // a no-op for filtered input, a defined result (the NA individuals dropped) otherwise.  Methylation data: p is used as given at
    // every individual below N, as the reference's meth dot_product (data.cpp:783-797) uses it -- its Ax leaves NA individuals
    // unmasked too, and its ATx must see them.
    if (!c->dense.resident) gvk::mask_copy(c->stream, c->w_n->d, c->w_n->d, c->mask2, c->npad);
    KCHK(c);
    if (atx_device(c, c->w_n->d, c->cg_d->d)) return 1;
    return to_host(c, out, c->cg_d->d, sizeof(double) * (c->M > 0 ? c->M : 0));
}

}  // extern "C"
