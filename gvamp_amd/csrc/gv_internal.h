// gv_internal.h -- context layout and kernel-launch prototypes shared by the libgvamp translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdint>
#include <memory>
#include <string>
#include <unordered_set>
#include <vector>

#include "gvamp.h"
#include "gv_mfma.h"

struct gv_vec {
    gv_ctx* ctx;
    int space;      // GV_SPACE_M / GV_SPACE_N
    int64_t len;    // logical length (M or 4*mbytes)
    int64_t cap;    // allocated doubles (M or npad); the tail beyond len is kept at 0
    double* d;
    bool owns = true;   // false: d points into another vector's allocation (w_n2 behind w_n)
};

// ---- fixed-point i8 MFMA route for 8-bit dosage codes (gv_dense_mfma.hip; gv_set_dosage_route) -----------------------------------
namespace gvdm {
// THE int32 invariant of the route: a K-entry adds at most 128 * 128 = 16 384 in magnitude to an int32 column sum of a streaming
// kernel, so no int32 accumulation spans more than SEG_MAX = (2^31 - 1) / 16 384 K-entries -- over the individuals in ATx, over the
// markers in Ax.  Longer sums are cut into segments whose int32 partials the epilogues add in int64 (cut() in gv_dense_mfma.hip).
constexpr int64_t SEG_MAX = 131071;
constexpr int ATX_KSTEP = 128, AX_KSTEP = 64;       // K-entries per step of the streaming kernels: a segment is a whole number of steps
constexpr int64_t PITCH_MAX = (int64_t)1 << 26;     // the Ax kernel keeps a lane's offset within 64 rows in 32 bits
constexpr int BLOCKS = 1024;                        // most blocks of a quantisation launch
// per-pass scratch, owned by DenseData: digits (16 bytes per K-entry), int32 partials, block maxima | limb sums | scalars
struct Scratch {
    void* dig = nullptr;
    size_t dig_cap = 0;
    int32_t* part = nullptr;
    size_t part_cap = 0;
    double* pmax = nullptr;
    long long* limb = nullptr;
    double* scal = nullptr;
};
struct Shape {
    int64_t blocks = 1;             // blocks of 128 rows (ATx: markers, Ax: individuals), one wave each
    int64_t steps = 1;              // K-steps in all
    int64_t seg_steps = 1;          // K-steps per segment
    int segs = 1;
};
}  // namespace gvdm

// The resident dense matrix of the dense kinds (gv_dense.hip): fp64 values of methylation data (gv_upload_meth / gv_upload_meth_file /
// gv_synth_meth; bits == 0) or unsigned 8- / 16-bit codes of compact dense data, X = scale * B (gv_upload_dosage /
// gv_upload_dosage_file / gv_synth_dosage).  One owner of the rows whatever the width; freed and reset by gvi::dense_release alone.
struct DenseData {
    void* rows = nullptr;           // M * pitch elements, marker-major, zeros in the padding
    int bits = 0;                   // 0 = doubles, 8 / 16 = codes of that width
    int64_t pitch = 0;              // elements per row: N rounded up to a multiple of 64
    bool resident = false;
    double scale = 1.0;             // codes only: the factor between codes and values
    double* mu = nullptr;           // codes only: M mean codes mu' (mave = scale * mu'): the products work in code units
    double* cnt = nullptr;          // codes only: M per-marker counts sum b na of the last gv_marker_stats (missing-aware kernels only)
    // codes only: M per-marker q = sum_present ((b - mu') na)^2 of the last gv_marker_stats, in code units -- the variance input of the
    // screens on dosage data (gv_set_screen_dosage: q == 0 is the marker without variance, sxx = scale^2 q)
    double* qss = nullptr;
    // missing entries: na = the codes were uploaded with gv_set_dosage_missing on; reserved = the reserved codes counted at that ingest
    // (device word rcount, block partials rpart)
    bool na = false;
    unsigned long long reserved = 0;
    unsigned long long *rcount = nullptr, *rpart = nullptr;
    double* part = nullptr;         // Ax partial vectors: 2 * segs * npad doubles
    size_t part_cap = 0;
    int cus = 0;                    // CU count of the device (the Ax decomposition's only input beyond N and M)
    gvdm::Scratch fx;               // 8-bit codes on the fixed-point route: digits and integer partials of a pass
    size_t elem_bytes() const { return bits ? (size_t)bits / 8 : sizeof(double); }
    size_t bytes(int64_t M) const { return elem_bytes() * (size_t)M * (size_t)pitch; }
};

// Grow-only device scratch of a batch product (gv_score_dev, gv_atxm_dev, gv_pca_dev): kept between calls, freed with the dataset
struct DevScratch {
    void* buf = nullptr;
    size_t cap = 0;
    void release() {
        if (buf) (void)hipFree(buf);
        buf = nullptr;
        cap = 0;
    }
    // at least `bytes` (the contents do not survive growing); false: the allocation failed and nothing is held
    bool reserve(size_t bytes) {
        if (bytes <= cap) return true;
        release();
        if (hipMalloc(&buf, bytes) != hipSuccess) {
            (void)hipGetLastError();
            buf = nullptr;
            return false;
        }
        cap = bytes;
        return true;
    }
};

// gv_score_dev: the fewest columns for which its own kernel is the path where it applies (measured: DESIGN.md section 21)
constexpr int GV_SCORE_MIN_COLS_DEFAULT = 4;
// gv_atxm_dev: the same for its kernel (measured: DESIGN.md section 23)
constexpr int GV_ATXM_MIN_COLS_DEFAULT = 4;
// ... and for its kernel on 8-bit dosage codes under the fixed-point route
constexpr int GV_ATXM_DENSE_MIN_COLS_DEFAULT = 3;

struct gv_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;

    // dataset ------------------------------------------------------------------------------------
    int64_t N = 0, M = 0, Mt = 0, S = 0;
    int64_t mbytes = 0;   // ceil(N/4)
    int64_t pitch = 0;    // bytes per marker row in HBM (multiple of 64)
    int64_t npad = 0;     // 4 * pitch : device length of every N-space vector
    uint8_t* bed = nullptr;     // M * pitch, marker-major 2-bit, pad bytes 0
    uint32_t* mask2 = nullptr;  // pitch/4 words: bits 2q and 2q+1 set iff individual 16j+q has a phenotype
    int64_t nonas = 0;
    double* mave = nullptr;
    double* msig = nullptr;
    uint32_t* counts = nullptr;     // 3*M: present individuals with a = 2, 1, 0 per marker (marker statistics)
    double alpha_scale = 1.0;       // of the last gv_marker_stats
    bool have_stats = false;
    // Defaults = the engine bench.py measures: i8 MFMA kernels on a re-encoded layout picked at ingest, no raw rows resident.
    // The fp64 VALU family (parity anchor) and the raw rows (gv_download_bed) are opt-in: gv_set_kernel_mode(ctx, 0),
    // gv_set_layout(ctx, 1, ..).
    int kernel_mode = 1;            // 0 = fp64 VALU on raw rows, 1 = i8 MFMA on stripes, 2 = the same in two-level fixed point (gvm::ax_wide)
    bool want_raw = false, want_stripes = true;  // layouts built at ingest (gv_set_layout)
    bool want_auto = true;                       // gv_set_layout(.., 3): want_tile is decided at ingest from the free HBM
    bool want_tile = false;                      // the MFMA family's layout: false = two stripe sets, true = one tile layout
    bool have_raw = false, have_stripes = false;
    gvm::Plan plan;
    // ticket counter of the streaming kernels (gv_mfma.h, gvm::Deal): allocated by gv_create unless GV_DEAL=0 (development: the
    // block-index mapping from the same binary), handed to the plan by plan_decomps; every streaming launch goes to `stream`
    gvm::Deal deal;
    // candidate work decompositions of the ATx-side / Ax-side streaming kernels (default first) and whether the on-device
    // pick among them has been made (autotune_ks)
    std::vector<gvm::Decomp> dec_cand_m, dec_cand_n;
    bool ks_fixed_m = false, ks_fixed_n = false;   // an override fixed the decomposition: nothing to pick
    bool ks_tuned = false;
    double ingest_alloc_s = 0.0, ingest_fill_s = 0.0;   // last ingest: allocating the resident layouts / filling them
    double ingest_overlap_s = 0.0;  // ... of which the allocation ran beside the preparation of the source (helper thread)
    size_t ingest_bytes = 0;        // bytes of genotype layouts resident after the last ingest
    int64_t expected_passes = 0;    // gv_set_expected_passes: 0 = unknown
    // the resident dense matrix (DenseData above).  While it is resident no genotype layout is, and every product dispatches on it
    // ahead of the kernel mode and the layout.
    DenseData dense;
    // missing entries of compact dense data (gv_set_dosage_missing): the all-ones code is a missing entry.  dosage_missing is the
    // setting, read by the next upload of codes; it outlives the dataset.  What the resident codes were uploaded with is dense.na;
    // the missing-aware kernels run when dosage_na_kernels(c) says so.
    bool dosage_missing = false;
    bool force_na_kernels = false;  // GV_DOSAGE_NA_KERNELS=1 (development, read by gv_create per context)
    // gv_set_dosage_route: the request (0 = the k_dosage_* VALU kernels, 1 = fixed-point i8 MFMA); it outlives the dataset.  What runs:
    // dosage_mfma_route(c).  dosage_seg: most K-entries per int32 segment of that route (GV_DOSAGE_MFMA_SEG, development, per context)
    int dosage_route = 0;
    int64_t dosage_seg = gvdm::SEG_MAX;
    double tune_seconds = 0.0;      // wall time the pick cost (0 when it came from the cache)
    int tune_source = 0;            // 0 model's first candidate, 1 measured, 2 cache, 3 fixed by an override / nothing to tune

    // workspaces ---------------------------------------------------------------------------------
    double* t3 = nullptr;          // 3*M: per-marker Ax table {(2-mu)c, (1-mu)c, (0-mu)c}
    double* ax_partial = nullptr;  // ax_chunks * npad
    int ax_chunks = 0;
    double* red_partial = nullptr; // RED_BLOCKS * RED_MAXK block partials
    double* red_out = nullptr;     // RED_MAXK device scalars
    double* host_pin = nullptr;    // pinned, RED_MAXK doubles
    // scalar mailbox: mapped coherent host memory the device writes into (k_publish), RED_MAXK doubles + a sequence flag
    double* mbox = nullptr;        // host address
    double* mbox_dev = nullptr;    // the same memory as the device sees it
    unsigned long long mbox_seq = 0;
    bool use_mbox = false;
    // a reduction whose finalisation publishes to the mailbox itself (arm_scalars -> gvk::arm_publish -> k_finalize_pub)
    unsigned int* pub_counter = nullptr;
    bool pub_armed = false;
    unsigned long long pub_seq = 0;
    void* xfer_pin = nullptr;      // 8 MiB pinned staging buffer of the whole-vector host transfers (to_host / to_device)
    hipEvent_t xfer_ev[4] = {nullptr, nullptr, nullptr, nullptr};   // to_host: one per 2 MiB piece of the staging buffer
    // device-resident CG (cg_run_device): 2 state blocks of gvm::ST_SIZE doubles, the `go` / rider flags, residual traces
    // (2 x cgx_relcap doubles), a pinned staging block for the initial states
    double* cgx_state = nullptr;
    int* cgx_go = nullptr;
    double* cgx_rel = nullptr;     // (device view of mapped, coherent HOST memory: the decide kernels write a trace entry per step straight
    double* cgx_rel_h = nullptr;   //  into it and the host reads it behind the status it already waits for -- no copy, no event)
    int cgx_relcap = 0;
    // How far the device-resident loops enqueue ahead of their statuses: the steps (cg_run_device) / passes (gv_cg_solve_aat2w) the
    // previous solve of the same kind needed.  From that count on the host reads the status of the step it has just enqueued before
    // it enqueues another -- consecutive VAMP iterations repeat their step counts, and a step enqueued after the last one costs a
    // dozen dropped launches (~60 us) where a wrong guess the other way costs one host round trip (~15 us).  0 = no hint yet.
    // The hint holds for TWO counts (hint, hint + 1): a solve that outgrows it (cg_iters 2 -> 27 -> 31 on LD genotypes) goes back to
    // reading one step behind, so the run-ahead is not lost for the rest of the solve.  One hint per solver kind (LMMSE alone,
    // Onsager alone, the two in lock-step; the joint N-space solver): a --fuse-solves 0 run alternates kinds with different counts.
    // Reset with the data set (free_dataset).
    int spec_hint_steps[3] = {0, 0, 0}, spec_hint_passes = 0;
    void* stripes_slab = nullptr;  // owner of plan.stripes_n | plan.stripes_m when the two stripe sets share one allocation (ingest)
    double* aat_slab = nullptr;    // work vectors of the N-space solvers (gv_solvers.hip: aat_scratch), kept between calls
    size_t aat_slab_cap = 0;
    gv_vec *mave_p = nullptr, *msig_p = nullptr, *numb_p = nullptr;   // people statistics (gv_people_stats), N-space
    // the people statistics belong to the data set, mask and marker statistics they were summed over: set by gv_people_stats, cleared
    // wherever have_stats is (gv_set_mask, gv_marker_stats, every ingest, free_dataset)
    bool have_people = false;
    gv_vec *w_n = nullptr, *w_n2 = nullptr;                  // N-space scratch (lmmse_mult, two-vector form)
    gv_vec *cg2_r = nullptr, *cg2_z = nullptr, *cg2_p = nullptr, *cg2_d = nullptr;   // second CG system (gv_cg_solve2)
    gv_vec *cg_r = nullptr, *cg_z = nullptr, *cg_p = nullptr, *cg_d = nullptr;  // CG work vectors
    std::unordered_set<gv_vec*> live_vecs;   // every vector of this context (vec_new / vec_del): freed at gv_destroy

    // LD-block preconditioner of the M-space CG solves (gv_set_cg_precond, gv_precond.hip).  Windows u in [pc_u0, pc_u0 + pc_nu)
    // overlap the shard; each holds a W x W block (zero beyond its clipped length).  Dropped with the data set, the mask and the
    // marker statistics (pc_invalidate).
    int pc_kind = 0, pc_W = 128;
    int64_t pc_u0 = 0, pc_nu = 0;
    double* pc_gram = nullptr;      // pc_nu * W * W: exact diagonal blocks of A^T A
    double* pc_inv = nullptr;       // pc_nu * W * W: (tau G + gam2 I)^-1 of the last factorisation
    int* pc_fail = nullptr;         // pc_nu flags of the last factorisation: 1 = the window fell back to the scalar rule
    bool pc_have_gram = false, pc_have_inv = false;
    double pc_tau = 0.0, pc_gam2 = 0.0, pc_build_s = 0.0;
    int64_t pc_factorisations = 0, pc_fallback = 0;
    gv_ld_stats ld_last{};          // gv_ld_info: the last gv_ld_scores / gv_ld_band call (gv_ld.hip)
    // gv_set_ld_dosage: gv_ld_scores / gv_ld_band accept resident 8-bit dosage codes; it outlives the dataset.
    // ld_dosage_edge: markers per side of a block of the one-product kernel, 64 or 128 (GV_LD_DOSAGE_EDGE, development, per context)
    int ld_dosage = 0;
    int ld_dosage_edge = 128;
    // gv_ld_scores_pos: the most bytes of per-block partial sums one pass may hold (GV_LD_PART_MB, development,
    // per context; a memory budget, not a tuned number) and the passes the last LD call took (gv_ld_last_passes)
    double ld_part_bytes = 2147483648.0;
    int ld_last_passes = 0;
    // gv_grm_apply: the most bytes of block terms one pass may hold (GV_GRM_PART_MB, development, per context)
    double grm_part_bytes = 2147483648.0;
    // gv_ld_clump: the rounds of the selection, |E1| and |E2| of the last call (gv_ld_clump_last), and the
    // seconds of its block pass and of its selection (gv_ld_clump_seconds)
    int clump_rounds = 0;
    int64_t clump_n_e1 = 0, clump_n_e2 = 0;
    double clump_block_s = 0.0, clump_select_s = 0.0;
    // gv_score_dev (gv_score.hip): scratch of the kernel path (grown on demand, freed with the dataset), the
    // development overrides GV_SCORE_COLS / GV_SCORE_KS (0: the library's pick), the fewest columns that take the kernel
    // (GV_SCORE_KERNEL=1 / 0: 1 / never) and what gv_score_info reports
    DevScratch score_scratch;
    int score_cols = 0, score_ks = 0;
    int score_min_cols = GV_SCORE_MIN_COLS_DEFAULT;
    gv_score_stats score_last{};
    // gv_atxm_dev (gv_atxm.hip): the same five for the ATx side (GV_ATXM_COLS / GV_ATXM_KS / GV_ATXM_KERNEL)
    DevScratch atxm_scratch;
    int atxm_cols = 0, atxm_ks = 0;
    int atxm_min_cols = GV_ATXM_MIN_COLS_DEFAULT;
    gv_atxm_stats atxm_last{};
    // ... on 8-bit dosage codes under the fixed-point route (gv_dense_atxm.hip): a threshold of its own, which
    // GV_ATXM_KERNEL=1 / 0 sets as it sets atxm_min_cols; GV_ATXM_COLS picks the columns per pass of either kernel
    int atxm_dense_min_cols = GV_ATXM_DENSE_MIN_COLS_DEFAULT;
    int atxm_dense_tiles = 0;       // GV_ATXM_TILES=4|8 (development, per context): tiles of 16 rows per wave; 0 = the library's pick
    // gv_set_screen_dosage: gv_screen_dev / gv_screen_cov_set / gv_screen_cov_dev accept resident dosage codes; it
    // outlives the dataset.  Read by every call: nothing is derived from it
    int screen_dosage = 0;
    // gv_pca_dev (gv_pca.hip): the work panels and small buffers (grown on demand, freed with the dataset) and what
    // gv_pca_info reports
    DevScratch pca_scratch;
    gv_pca_stats pca_last{};
    gv_king_stats king_last{};      // gv_king_info: the last gv_king_block / gv_king_pairs call (gv_king.hip)
    gv_grm_stats grm_last{};        // gv_grm_info: the last gv_grm_weights / gv_grm_block / gv_grm_pairs call (gv_grm.hip, section 28)
    // gv_screen_cov_set / gv_screen_cov_dev (gv_screen_cov.hip): the cached state of the covariate side -- the
    // orthonormal basis Q (cov_K columns of npad doubles) and behind it v (M doubles), in an allocation of its own (the work panels of
    // both calls are pca_scratch's).  It belongs to the data set, mask and marker statistics it was computed from: have_cov is cleared
    // wherever have_stats is cleared or set anew (cov_drop: gv_set_mask, gv_marker_stats, every ingest, free_dataset, which also frees it)
    DevScratch cov_cache;
    bool have_cov = false;
    int cov_K = 0;
    gv_screen_cov_stats cov_last{};

    // communicator ---------------------------------------------------------------------------------
    ncclComm_t comm = nullptr;
    std::shared_ptr<void> comm_keep;       // owns comm: ncclCommDestroy when the last context sharing it lets go (gv_comm_share)
    int rank = 0, nranks = 1;
    void* local = nullptr;                 // in-process test communicator (gv_comm_init_local)
    std::shared_ptr<void> local_keep;
    std::vector<double> local_buf;
    int overlap_tiles = 0;                 // > 1: data::Ax in that many individual chunks, exchange on comm_stream (GV_OVERLAP)
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_chunk = nullptr, ev_comm = nullptr;
    gv_allreduce_fn cb = nullptr;          // host-callback communicator (gv_comm_init_callback)
    void* cb_user = nullptr;
    // gv_debug_force_multi: a ONE-rank context takes every multi-rank branch; the exchange is an in-stream loop-back through
    // scratch (1), the 1-rank RCCL communicator (2) or both (3) -- never a host synchronisation
    int force_multi = 0;
    int loop_delay_us = 0;
    double* loop_buf[2] = {nullptr, nullptr};     // [0] the context's stream, [1] the side stream of the overlapped exchange
    size_t loop_cap[2] = {0, 0};

    // instrumentation ------------------------------------------------------------------------------
    int timing = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    gv_counters cnt{};
    struct EvRec { hipEvent_t a, b; int kind; };
    std::vector<EvRec> ev_pool;   // timing == 2: un-synchronised event pairs around the matvec kernels
    size_t ev_used = 0;
};

// (RED_BLOCKS: gv_mfma.h, beside the stride of the prep launches' block partials)
constexpr int RED_MAXK = 80;   // >= 1 + 2*(LMAX-1) with LMAX = 32
constexpr int GV_LMAX = 32;

struct gv_prior {
    int L;
    double probs[GV_LMAX];
    double vars[GV_LMAX];
};

// ---- kernel launchers (gv_kernels.hip) -----------------------------------------------------------
namespace gvk {
void synth_bed(hipStream_t s, uint8_t* bed, int64_t M, int64_t S, int64_t N, int64_t pitch, uint64_t seed,
               uint32_t miss_thr, uint32_t ld_block = 0, uint32_t ld_thr = 0);
void marker_stats(hipStream_t s, const uint8_t* bed, const uint32_t* mask2, int64_t M, int64_t pitch, double nonas,
                  double alpha_scale, double* mave, double* msig, uint32_t* counts);
void marker_sums2_f64(hipStream_t s, const uint8_t* bed, int64_t M, int64_t pitch, const double* p1, const double* p2,
                      double* out4);
void people_table(hipStream_t s, const double* mave, const double* msig, int64_t M, int kind, double* t3);
void people_finish(hipStream_t s, double* s1, double* s2, const double* cnt, const uint32_t* mask2, int64_t N,
                   int64_t npad);
void aat_diag(hipStream_t s, const double* mave_p, const double* msig_p, const double* numb_p, double tau, double gam2,
              double Nd, int64_t npad, double* diag);
void cg_step_b_diag(hipStream_t s, double* r, const double* d, double alpha, const double* diag, double* z, int64_t n,
                    double* partial, double* out);   // out = <r,z>, <r,r>
void probit_denoise(hipStream_t s, const double* p1, const double* y, const double* m_cov, int64_t N, int64_t npad,
                    double tau1, double probit_var, double* z1, double* partial, double* out);   // out = sum g1d, sum (z1-p1)^2
// --model robust: out = sum dz1/dp1, sum (z1-p1)^2 ; delta_H objective: out[g] = sum_n E[rho_{grid[g]}(y_n - z)], z ~ N(p1_n, 1/tau1)
constexpr int HUBER_GMAX = 16;
struct HuberGrid { double v[HUBER_GMAX]; };
void huber_denoise(hipStream_t s, const double* p1, const double* y, int64_t N, int64_t npad, double tau1, double deltaH,
                   double* z1, double* partial, double* out);
void huber_delta(hipStream_t s, const double* p1, const double* y, int64_t N, double tau1, const HuberGrid& grid, int G,
                 double* partial, double* out);
void mul(hipStream_t s, double* out, const double* x, const double* y, int64_t n);
void select_eq(hipStream_t s, double* out, const double* x, const int* key, int value, int64_t n);
void ax_table(hipStream_t s, const double* x, const double* mave, const double* msig, int64_t M, double* t3);
void ax_f64(hipStream_t s, const uint8_t* bed, int64_t M, int64_t pitch, const double* t3, int chunks,
            double* partial, int64_t npad);
void ax_reduce(hipStream_t s, const double* partial, int chunks, int64_t npad, const uint32_t* mask2, double scale,
               double* out);
void scale_vec(hipStream_t s, double* v, int64_t n, double a);
void atx_f64(hipStream_t s, const uint8_t* bed, int64_t M, int64_t pitch, const double* p, const double* mave,
             const double* msig, double scale, double* out);
void fill(hipStream_t s, double* v, int64_t n, double a);
void fill_hash(hipStream_t s, double* v, int64_t n, uint64_t seed);
void publish(hipStream_t s, const double* src, int K, double* mailbox, unsigned long long* flag, unsigned long long seq);
// the finalisation of the NEXT reduction launched from this thread also publishes its scalars (no k_publish launch)
void arm_publish(double* mailbox, unsigned long long* flag, unsigned long long seq, unsigned int* counter);
void disarm_publish();
void axpby(hipStream_t s, double* out, double a, const double* x, double b, const double* y, int64_t n);
void mask_copy(hipStream_t s, double* out, const double* in, const uint32_t* mask2, int64_t npad);
void copy(hipStream_t s, double* dst, const double* src, int64_t n);                  // dst = src (kernel, not hipMemcpyAsync)
void p_update(hipStream_t s, double* p, const double* z, double beta, int64_t n);     // p = fma(beta, p, z)
// one-rank all-reduce that moves the message through scratch and poisons it meanwhile (gv_debug_force_multi)
void loopback(hipStream_t s, double* buf, double* scratch, int64_t n, int delay_us);
// K dot products <x[k], y[k]> over n elements -> red_out[0..K)
void dots(hipStream_t s, int K, const double* const* x, const double* const* y, int64_t n, double* partial,
          double* out);
void dots_ex(hipStream_t s, int K, const double* const* xa, const double* const* xb, const double* const* ya,
             const double* const* yb, const int64_t* n, double* partial, double* out);   // <xa - xb, ya - yb>, lengths n[k]
// device-resident CG step (gv_solvers.hip: cg_run_device)
// dp_part != NULL (one rank): <d,p> of system k is still in dp_nb block partials at dp_part[k] and the three sums of this
// launch stay block partials too (k_cgx_decide adds them up: cgx_decide's part / part_nb); returns the number of blocks
int cgx_ab(hipStream_t s, int nsys, double* const* st, double* const* mu, const double* const* p, const double* const* v,
           double* const* r, const double* const* d, double* const* z, const double* const* dp, double* const* part,
           double* const* red, double diag, int64_t n, const double* const* dp_part = nullptr, int dp_nb = 0,
           double* const* az = nullptr, const double* const* aw = nullptr, int64_t npad = 0);   // az: A mu += alpha A p rides along
void finalize(hipStream_t s, const double* partial, int nb, int K, double* out);   // ordered sum of block partials
void state_init(hipStream_t s, double* dst, const double* q);   // q: gvm::ST_SIZE doubles, by value in the launch
void set_ints(hipStream_t s, int* dst, int a, int b);
void go_from_states(hipStream_t s, int* dst, const double* st0, const double* st1, int b);
// the state block of a system at its start from the block partials of its two opening reductions over n entries (one rank)
void state_from_partials(hipStream_t s, double* dst, const double* q, const double* part_rz, int K_rz, int k_rz, const double* part_vv,
                         int64_t n, bool sqrt_norm);
void state_from_scalars(hipStream_t s, double* dst, const double* q, const double* rz, const double* vv, bool sqrt_norm);
void cgx_decide(hipStream_t s, int nsys, double* const* st, const double* const* red, double* const* relres, double gam2,
                int max_iter, int* go, double* mailbox, unsigned long long* flag, unsigned long long seq, int* ride,
                const double* other_st = nullptr, const int* ride_report = nullptr, const double* const* part = nullptr,
                int part_nb = 0);
void ride_mark(hipStream_t s, const double* st0, const double* st1, int* ride);
void p_update_st(hipStream_t s, double* p, const double* z, const double* st, int64_t n);   // p = z + beta p while st is stepping
void aat_step(hipStream_t s, double* st, double* mu, double* p, double* r, double* d, double* z, const double* diag, double tau,
              double gam2, int64_t n, double* partial, double* relres, int max_iter, double* mailbox,
              unsigned long long* flag, unsigned long long seq, double* at_acc = nullptr,
              const double* at_p = nullptr, int64_t m = 0, const double* other_st = nullptr, int* go = nullptr,
              const int* ride = nullptr, int* ride_mark = nullptr, bool p_update = true, bool dq_done = false);
void ride_copy(hipStream_t s, double* out, const double* w0, const double* w1, const double* st0, const double* st1,
               const int* ride, int64_t n);
void cg_step_a(hipStream_t s, double* mu, const double* p, double alpha, const double* v, int64_t n,
               double* partial, double* out);                 // mu += alpha p ; out[0] = <v, mu>
void cg_step_b(hipStream_t s, double* r, const double* d, double alpha, double diag, double* z, const double* mu,
               int64_t n, double* partial, double* out);      // r -= alpha d ; z = r/diag ; out = <r,z>,<z,z>,<r,r>,<mu,mu>
void denoise(hipStream_t s, const double* r1, int64_t n, double gam1, const gv_prior& pr, double* x1, double* dd,
             double* partial, double* out);                   // out[0] = sum g1d, out[1] = sum (x1-r1)^2
void prior_estep(hipStream_t s, const double* r1, int64_t n, double gam1, double lambda, const gv_prior& om_vars,
                 double* partial, double* out);               // out[0..1+2(L-1))
void pvals_test(hipStream_t s, const uint32_t* cnt, const double* mave, const double* msig, const double* sums4,
                const double* xself, double self_scale, const int* chrom, int ch, int64_t M, double* pvals, double* beta = nullptr,
                double* se = nullptr, double* tstat = nullptr);      // beta / se / tstat: all three (gv_assoc_*) or none
void copy_bw(hipStream_t s, const double* src, double* dst, int64_t n);
void read_bw(hipStream_t s, const void* src, int64_t blocks_per_wave, int64_t nwaves, unsigned int* sink, int perm = 0);
}  // namespace gvk

// ---- the dense kinds: fp64 design matrix and 8- / 16-bit codes (gv_dense.hip) ----------------------------------------------------
namespace gvd {
int64_t row_pitch(int64_t N);       // elements per resident row: N rounded up to 64
struct AxShape {
    int64_t col_tiles = 1;          // workgroups across the individuals
    int64_t seg_len = 1;            // markers per segment
    int segs = 1;                   // marker segments = partial vectors
};
constexpr int AX_COLS_F64 = 512;
int ax_cols(int bits);              // individuals per Ax workgroup: 512 (fp64, bits == 0), 4096 (8-bit codes), 2048 (16-bit codes)
AxShape ax_shape(int64_t N, int64_t M, int cus, int cols = AX_COLS_F64);
// What every kernel call on the resident matrix repeats (gvi::dense_view builds it from the context).  bits selects the kernels: 0 the
// fp64 kernels, 8 / 16 the kernels of that code type, na their missing-aware instantiation (gv_set_dosage_missing: the all-ones code
// is a missing entry).
struct View {
    void* rows;                     // M * pitch doubles or codes
    int bits;
    bool na;
    int64_t M, N, pitch;
    double* centre;                 // what a kernel subtracts per row: mave (fp64), the mean codes mu' (codes)
    double* msig;
    double wscale;                  // the factor between codes and values; 1 for fp64
    double* cnt;                    // codes: M per-marker counts sum b na, written by stats and read by assoc when na is set
    double* qss;                    // codes: M per-marker q = sum ((b - mu') na)^2, written by stats (DenseData::qss)
};
// the device-generated matrix of the rows [S, S + M); miss_thr: codes with na set only (gv_synth_dosage_na)
void synth(hipStream_t s, const View& v, int64_t S, uint64_t seed, uint64_t miss_thr = 0);
// gv_synth_dosage_ld (codes only): block-correlated columns, ld_block >= 1 markers per block, ld_thr = ld_ppm 2^32 / 10^6
void synth_ld(hipStream_t s, const View& v, int64_t S, uint64_t seed, uint64_t miss_thr, uint64_t ld_block, uint64_t ld_thr);
// marker statistics: mave, v.msig (codes: v.centre and, with na, v.cnt beside them; fp64: mave is v.centre)
void stats(hipStream_t s, const View& v, const uint32_t* mask2, double nonas, double alpha_scale, double* mave);
// out[m] = msig[m] sum_j (x[m][j] - mave[m]) p[j] * scale, then tau * out + gam2 * addx when addx != NULL (nv = 1 or 2 vectors)
void atx(hipStream_t s, int nv, const View& v, const double* pa, const double* pb, double scale, double* outa, double* outb,
         const double* addxa, const double* addxb, double tau, double gam2);
// partial[v][seg][j] over the segments of sh, then out[j] = scale * sum_seg partial (j < N), 0 at j >= N
void ax_partial(hipStream_t s, int nv, const AxShape& sh, const View& v, const double* va, const double* vb, double* part, int64_t npad);
void ax_reduce(hipStream_t s, int nv, const AxShape& sh, const double* part, int64_t N, int64_t npad, double scale, double* outa,
               double* outb);
// *total += the reserved codes among the pitched rows [m0, m0 + mc) of codes; partial: COUNT_BLOCKS device words of scratch
constexpr int COUNT_BLOCKS = 1024;
void count_reserved(hipStream_t s, const View& v, int64_t m0, int64_t mc, unsigned long long* partial, unsigned long long* total);
// gv_assoc_* on compact dense data.  assoc_prep: p[npad] = y - z1 (+ add when not NULL) at the individuals with a phenotype, 0 at NA and
// pad slots; sums[0..2) = {sum p, sum p^2} through the block partials (>= 2 * RED_BLOCKS doubles) in a fixed order.  assoc: the test of
// the rows rows[0..nrows) (NULL: rows 0..nrows) against p; beta / se / tstat / pval are M-space device vectors written at the tested
// rows only.  xself != NULL (leave-one-out): the row's own effect xself[m] * self_scale is added back analytically.
void assoc_prep(hipStream_t s, const double* y, const double* z1, const double* add, const uint32_t* mask2, int64_t npad, double* p,
                double* partial, double* sums);
void assoc(hipStream_t s, const View& v, const int64_t* rows, int64_t nrows, const double* p, const uint32_t* mask2, const double* psums,
           double nonas, const double* xself, double self_scale, double* beta, double* se, double* tstat, double* pval);
}  // namespace gvd

// ---- the fixed-point route of 8-bit codes (gv_dense_mfma.hip): NA = false views only ---------------------------------------------
namespace gvdm {
Shape atx_shape(int64_t N, int64_t M, int cus, int64_t cap);      // cap: most K-entries per int32 segment (<= SEG_MAX)
Shape ax_shape(int64_t N, int64_t M, int cus, int64_t cap);
hipError_t reserve(Scratch& w, int64_t N, int64_t M, int cus, int64_t cap);      // scratch for both products of this shape
void release(Scratch& w);
// gvd::atx / gvd::ax_partial + ax_reduce with the same arguments and meaning; ev0 / ev1 (may be NULL) are recorded around the
// streaming kernel
void atx(hipStream_t s, int nv, const gvd::View& v, const Scratch& w, const Shape& sh, const double* pa, const double* pb, double scale,
         double* outa, double* outb, const double* addxa, const double* addxb, double tau, double gam2, hipEvent_t ev0, hipEvent_t ev1);
void ax(hipStream_t s, int nv, const gvd::View& v, const Scratch& w, const Shape& sh, const double* xa, const double* xb, int64_t npad,
        double post, double* outa, double* outb, hipEvent_t ev0, hipEvent_t ev1);
// the quantisation of an ATx pass of one (pb == NULL) or two vectors of n entries into w.dig, with w.pmax / w.limb / w.scal
void quantise_atx(hipStream_t s, const double* pa, const double* pb, int64_t n, const Scratch& w);
int quant_blocks_of(int64_t n);       // the blocks whose limb sums that quantisation leaves
// gv_dense_atxm.hip: one pass of the batch product over ncols <= cp columns (cp = 4 or 8: the instantiation), out[j] = gvdm::atx of
// p[j] alone bit for bit.  sh = atx_shape(..); the buffers are the caller's (gv_dense_atxm_plan.h: cp / 2 pairs of pair_dig_bytes of
// digits and of pair_small_bytes of maxima, limb sums and scalars; sh.segs * sh.blocks * 128 * cp * 8 int32 partials); tiles: 4 or 8
// tiles of 16 rows per wave, 0 = atxm_tiles(cp)
hipError_t atxm_pass(hipStream_t s, const gvd::View& v, const Shape& sh, int cp, int tiles, int ncols, const double* const* p, double* const* out,
                     double scale, char* dig, size_t pair_dig_bytes, int32_t* part, char* small, size_t pair_small_bytes);
int atxm_tiles(int cp);               // the library's pick of the tiles per wave for that instantiation
}  // namespace gvdm

// ---- LD-block preconditioner (gv_precond.hip; the window Grams are an epilogue of the LD block kernel, gv_ld.hip) --------------
namespace gvp {
int64_t first_window(int64_t S, int W);             // first half-grid window u overlapping the shard [S, S+M)
int64_t num_windows(int64_t S, int64_t M, int W);
// out[u - first_window] = the W x W Gram of every window, zero beyond its clipped length (memset and one kernel on s)
void gram(hipStream_t s, const void* lay, int layout, int64_t nkb, const uint32_t* mask2, int64_t P4, int64_t N, int64_t S, int64_t M,
          int W, const double* mave, const double* msig, double* out);
// the same for resident 8-bit dosage codes under gv_set_ld_dosage: out = c's pc_nu x W x W device buffer, W = pc_W;
// scratch of its own, freed on return; returns after the kernels have run
int gram_dosage(gv_ctx* c, double* out);
int factor(hipStream_t s, const double* gram, int W, int64_t S, int64_t M, double tau, double gam2, double diag, double* inv, int* fail);
void apply(hipStream_t s, const double* inv, int W, int64_t S, int64_t M, const double* r, double* z);
}  // namespace gvp

// ---- internals shared by the translation units of the C ABI: gv_capi.hip (context, vectors, scalar mailbox), gv_comm.hip,
// gv_xfer.hip, gv_tune.hip, gv_matvec.hip, gv_ingest.hip, gv_stats.hip, gv_solvers.hip, gv_precond.hip ----------------------
namespace gvi {
int fail(gv_ctx* c, const char* fmt, ...);
int vec_new(gv_ctx* c, int space, gv_vec** out);
void vec_del(gv_ctx* c, gv_vec* v);
// a vector an entry point may read or write M / npad doubles through: of this context, of that space, and of the length and capacity
// vec_new would give it NOW (a caller's vector that survived gv_set_dims keeps those of the earlier dimensions)
inline bool vec_ok(const gv_ctx* c, const gv_vec* v, int space) {
    return v && v->ctx == c && v->space == space && v->len == (space == GV_SPACE_M ? c->M : 4 * c->mbytes) &&
           v->cap == (space == GV_SPACE_M ? (c->M > 0 ? c->M : 1) : c->npad);
}
// vec_ok as a refusal: the message names the entry point, the argument and what is wrong with it.  space < 0: the vector's own
int vec_need(gv_ctx* c, const char* who, const char* arg, const gv_vec* v, int space = -1);
int ensure_w2(gv_ctx* c);       // the second N-space scratch vector (behind w_n in one allocation)
int ensure_work(gv_ctx* c);     // scratch vectors of the matvecs and the CG
int read_scalars(gv_ctx* c, int K, double* out);                            // red_out[0..K) -> host (mailbox or copy)
// Call right before launching a reduction (gvk::dots, cg_step_*, denoise, ...) whose red_out[0..K) the very next
// read_scalars(c, K, .) fetches, with nothing all-reduced in between: saves the k_publish launch of that read-back.
void arm_scalars(gv_ctx* c);
int read_scalars_global(gv_ctx* c, int K, double* out, bool multi);         // the same, summed over the ranks first
int allreduce_scalars(gv_ctx* c, double* buf, int K);                       // MPI_Allreduce(SUM) of K host scalars
bool is_multi(const gv_ctx* c);
int comm_allreduce(gv_ctx* c, double* dev, size_t n);
int comm_allreduce_on(gv_ctx* c, double* dev, size_t n, hipStream_t stream);
int to_host(gv_ctx* c, void* dst, const void* src_dev, size_t nbytes);
int to_device(gv_ctx* c, void* dst_dev, const void* src, size_t nbytes, bool sync = true);
// data::Ax / data::ATx on device pointers, nv = 1 or 2 vectors, in the kernel family of the context (gv_matvec.hip)
// (cg: the slots of the pass that belong to a CG system with device-resident scalars -- gvm::CgHook; kernel mode 1 only)
int ax_pass(gv_ctx* c, int nv, const double* xa, const double* xb, double* outa, double* outb, const gvm::CgHook* cg);
int atx_pass(gv_ctx* c, int nv, const double* pa, const double* pb, double* outa, double* outb, const double* addxa,
             const double* addxb, double tau, double gam2, const gvm::CgHook* cg);
inline int ax_device(gv_ctx* c, const double* x, double* out, const gvm::CgHook* cg = nullptr) {
    return ax_pass(c, 1, x, nullptr, out, nullptr, cg);
}
inline int atx_device(gv_ctx* c, const double* p, double* out, const double* addx = nullptr, double tau = 1.0, double gam2 = 0.0,
                      const gvm::CgHook* cg = nullptr) {
    return atx_pass(c, 1, p, nullptr, out, nullptr, addx, nullptr, tau, gam2, cg);
}
inline int ax2_device(gv_ctx* c, const double* xa, const double* xb, double* outa, double* outb, const gvm::CgHook* cg = nullptr) {
    return ax_pass(c, 2, xa, xb, outa, outb, cg);
}
inline int atx2_device(gv_ctx* c, const double* pa, const double* pb, double* outa, double* outb, const double* addxa = nullptr,
                       const double* addxb = nullptr, double tau = 1.0, double gam2 = 0.0, const gvm::CgHook* cg = nullptr) {
    return atx_pass(c, 2, pa, pb, outa, outb, addxa, addxb, tau, gam2, cg);
}
int lmmse_device(gv_ctx* c, const double* v, double tau, double gam2, double* out);
bool use_overlap(const gv_ctx* c);    // data::Ax cut into chunks whose exchange runs on the side stream (GV_OVERLAP)
int ax_overlapped(gv_ctx* c, int nv, const double* xa, const double* xb, double* outa, double* outb, const gvm::CgHook* cg);
int autotune_ks(gv_ctx* c);     // picks the work decompositions of the streaming kernels (once per shard)
int plan_decomps(gv_ctx* c);    // geometry and candidate decompositions for the layout that will be built (gv_set_dims, ingest)
void ev_resolve(gv_ctx* c);     // timing == 2: the pending event pairs into the counters
// kind 1 of gv_set_cg_precond: Grams built and (tau, gam2) factorised, ready for pc_apply (error when that cannot be)
int pc_prepare(gv_ctx* c, double tau, double gam2);
void pc_apply(gv_ctx* c, const double* r, double* z);
void pc_invalidate(gv_ctx* c, bool free_mem);
// what the exact blocks of A^T A need (gv_ld.hip): not compact dosage data, not dense, a re-encoded layout, marker statistics and mask
// words, N within the int32 sums -- refused by message under the caller's name `who`, `why` being its reason for wanting genotypes
int planes_check(gv_ctx* c, const char* who, const char* why);
// gv_set_ld_dosage is on and compact dosage data are resident: the section-17 / 18 kernels answer (8-bit codes) or refuse (16-bit codes)
inline bool ld_dosage(const gv_ctx* c) { return c->ld_dosage && c->dense.resident && c->dense.bits != 0; }
// gv_set_screen_dosage is on and compact dosage data are resident: the screens accept the context (methylation data stay refused)
inline bool screen_dosage(const gv_ctx* c) { return c->screen_dosage && c->dense.resident && c->dense.bits != 0; }
// ... and what the Gram build needs of them: 8-bit codes, the mask, marker statistics, N within the 128-bit epilogue
int gram_dosage_check(gv_ctx* c, const char* who);
// compact dense data: the missing-aware kernels run when the codes were uploaded with gv_set_dosage_missing on AND the ingest counted a
// reserved code in this shard (a shard without one gets the same bits from the plain kernels) or GV_DOSAGE_NA_KERNELS=1 forces them
inline bool dosage_na_kernels(const gv_ctx* c) { return c->dense.na && (c->dense.reserved != 0 || c->force_na_kernels); }
// the fixed-point route is in force: requested, 8-bit codes resident, the NA = false kernels would run (and the pitch within the Ax
// kernel's 32-bit lane offsets); otherwise the k_dosage_* kernels run
inline bool dosage_mfma_route(const gv_ctx* c) {
    return c->dosage_route == 1 && c->dense.resident && c->dense.bits == 8 && !dosage_na_kernels(c) && c->dense.pitch <= gvdm::PITCH_MAX;
}
// the resident dense matrix as the gvd:: launchers take it
inline gvd::View dense_view(const gv_ctx* c) {
    const DenseData& d = c->dense;
    return {d.rows, d.bits, dosage_na_kernels(c), c->M, c->N, d.pitch, d.bits ? d.mu : c->mave, c->msig, d.bits ? d.scale : 1.0, d.cnt, d.qss};
}
// Frees the dense matrix with everything that belongs to it and resets its state: whatever kind comes next starts without a missing
// code and with no reserved code counted.  keep_alloc: the allocations stay for an upload of the same width (shape is the context's).
void dense_release(gv_ctx* c, bool keep_alloc = false);
// frees the genotype layouts of the MFMA family: the stripe slab, the two stripe sets, the tiles and the plan's digit / weight / sum buffers
void free_layouts(gv_ctx* c);
// The batch products (gv_score.hip, gv_atxm.hip).  batch_args: the checks their entry points make on C > 0 columns of handles -- `in`
// (named in_name in the messages) of in_space, `out` of the other space, of this context and its dimensions, the outputs distinct from
// each other and from the inputs -- and the device pointers behind them.  batch_host: the host-pointer form -- the C columns of `in`
// (one vector of in_space after the other) staged into fresh vectors (mask_in: masked as gv_atx masks its own), dev() on them, the C
// result columns copied to `out`, the stream synchronised, and the wall time of it all in *seconds
int batch_args(gv_ctx* c, const char* who, int64_t C, const gv_vec* const* in, gv_vec* const* out, const char* in_name, int in_space,
               std::vector<const double*>& is, std::vector<double*>& os);
int batch_host(gv_ctx* c, const char* who, int64_t C, const double* in, int in_space, bool mask_in, double* out,
               int (*dev)(gv_ctx*, int64_t, const gv_vec* const*, gv_vec* const*), double* seconds);
// gv_score.hip: Z = A W on device pointers (C > 0 columns, x[j] M doubles, out[j] npad doubles)
int score_device(gv_ctx* c, int64_t C, const double* const* x, double* const* out);
// gv_atxm.hip: R = A^T Y on device pointers (C > 0 columns, p[j] npad doubles, out[j] M doubles)
int atxm_device(gv_ctx* c, int64_t C, const double* const* p, double* const* out);
// gv_pca.hip: its panel kernels for the other files that work on panels of L <= GV_PCA_MAX_BLOCK separate fp64 columns of npad doubles
// (gv_screen_cov.hip).  The small buffers are the caller's (panel_bufs_bytes of device memory, 256-byte aligned); every array of column
// pointers holds L valid columns.  panel_gram: b.S = X^T Y, LM x LM row-major with LM = L <= 16 ? 16 : 32, through k_pca_gram and
// k_pca_gram_fin; an entry's summation order is a function of npad alone.  panel_orth: X <- orth(X) in place, CholeskyQR applied twice
// (k_pca_gram, k_pca_small in Cholesky mode, k_pca_apply); *b.flag, zeroed by the caller, is set to 1 by a pivot that is not positive
struct PanelBufs { double *part, *S, *W, *theta; int* flag; };
size_t panel_bufs_bytes();
PanelBufs panel_bufs_carve(char* base);
void panel_gram(gv_ctx* c, const PanelBufs& b, double* const* X, double* const* Y, int L);
void panel_orth(gv_ctx* c, const PanelBufs& b, double* const* X, int L);
// the cached state of gv_screen_cov_set is no longer that of the context's mask and marker statistics
inline void cov_drop(gv_ctx* c) {
    c->have_cov = false;
    c->cov_K = 0;
}

struct Timer {
    gv_ctx* c;
    double* acc;
    bool on;
    Timer(gv_ctx* c_, double* acc_) : c(c_), acc(acc_), on(c_->timing == 1) {
        if (on) (void)hipEventRecord(c->ev0, c->stream);
    }
    void stop() {
        if (!on) return;
        (void)hipEventRecord(c->ev1, c->stream);
        (void)hipEventSynchronize(c->ev1);
        float ms = 0;
        (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
        *acc += ms;
        on = false;
    }
};
}  // namespace gvi

#define HIPCHK(c, call)                                                                      \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) return fail(c, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define NCCLCHK(c, call)                                                                     \
    do {                                                                                     \
        ncclResult_t r_ = (call);                                                            \
        if (r_ != ncclSuccess) return fail(c, "%s failed: %s (%s:%d)", #call, ncclGetErrorString(r_), __FILE__, __LINE__); \
    } while (0)
#define KCHK(c) HIPCHK(c, hipGetLastError())
#define NEED(c, cond, msg)                 \
    do {                                   \
        if (!(cond)) return fail(c, msg);  \
    } while (0)
// a gv_vec argument of an entry point (vec_ok); NEED_VEC_OPT: it may be NULL
#define NEED_VEC(c, who, v, space)                                  \
    do {                                                            \
        if (gvi::vec_need(c, who, #v, v, space)) return 1;          \
    } while (0)
#define NEED_VEC_OPT(c, who, v, space)                              \
    do {                                                            \
        if ((v) && gvi::vec_need(c, who, #v, v, space)) return 1;   \
    } while (0)
// an entry point the dense kinds refuse, when the resident dataset is compact dense data (the fp64 kind keeps its own message)
#define REFUSE_DOSAGE(c, who, why)                                                                                      \
    do {                                                                                                                \
        if ((c)->dense.resident && (c)->dense.bits)                                                                     \
            return fail(c, "%s: not available for compact dosage data (%d-bit codes): %s", who, (c)->dense.bits, why); \
    } while (0)

