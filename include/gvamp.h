/* gvamp.h -- C ABI of libgvamp.so: the MI355X (gfx950) engine behind gVAMP's `class data` / `class vamp`
 * seam for the linear model.
 *
 * The reference has no plugin ABI; its seam is the C++ class `data` handed to `vamp` by pointer
 * (/root/reference/vamp.hpp:85-143, data.hpp:93-140).  Each entry point below names the reference
 * interface it replaces.  INTEGRATION.md shows the reference-side binding (a `data` subclass whose
 * Ax/ATx forward here).
 *
 * Conventions: every function returns 0 on success, non-zero on failure (message via gv_last_error);
 * no exceptions cross the ABI; all `const T*` / `T*` arguments are caller-owned HOST memory unless the
 * parameter is a gv_vec handle (device-resident fp64 vector owned by the context).  One context = one
 * marker shard on one GPU (the reference: one MPI rank, utilities.cpp:259-291).  Not thread-safe per
 * context; different contexts may be driven from different threads.
 *
 * There is NO CPU fallback: without a usable HIP device gv_create fails.
 */
#ifndef GVAMP_H
#define GVAMP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gv_ctx gv_ctx;
typedef struct gv_vec gv_vec;

/* Bumped whenever a struct of this header grows or a default changes, so that a binding compiled against an older header fails
 * its version check instead of overrunning a buffer.  History: 1 rounds 1-2; 2 round 3 (gv_decomp_info grew by whole_quads,
 * the context defaults became kernel mode 1 / no raw rows / layout auto) and round 4 (gv_ingest_info2, gv_set_expected_passes);
 * 3 round 5 (gv_cg_solve_aat2w takes v_a as the in/out vector it is; layout auto takes ONE resident layout unless the caller
 * announces a long run -- gv_set_expected_passes; gv_debug_force_multi); 4 round 6 (gv_decomp_info grew by wgs_per_cu and xcd_skew;
 * gv_set_kernel_mode accepts 2, the two-level fixed point).
 * A binding checks  gv_abi_version() == GV_ABI_VERSION  once, before anything else (INTEGRATION.md section B does). */
#define GV_ABI_VERSION 4

/* ---- context ------------------------------------------------------------------------------------ */
int gv_abi_version(void);
/* device: HIP ordinal.  Replaces nothing in the reference (it has no device boundary). */
int gv_create(int device, gv_ctx** out);
void gv_destroy(gv_ctx* ctx);
/* ctx may be NULL: returns the message of the last failed gv_create on this thread. */
const char* gv_last_error(const gv_ctx* ctx);
int gv_synchronize(gv_ctx* ctx);

/* ---- dataset: `data` constructors (data.cpp:30-113) ------------------------------------------------
 * N individuals, M local markers, Mt total markers, S first local marker (divide_work, utilities.cpp:259). */
int gv_set_dims(gv_ctx* ctx, int64_t N, int64_t M, int64_t Mt, int64_t S);
int64_t gv_mbytes(const gv_ctx* ctx);  /* ceil(N/4), data.cpp:40 */
/* bed: M*mbytes bytes, marker-major PLINK 2-bit, WITHOUT the 3 magic bytes: what read_genotype_data
 * (data.cpp:201-234) leaves in bed_data.  Copied to HBM (row pitch padded to 64 B) and kept resident. */
int gv_upload_bed(gv_ctx* ctx, const uint8_t* bed, size_t nbytes);
/* The same from a file, streamed through a bounded pinned buffer (host memory stays O(8192 * mbytes) however large
 * the shard): M*mbytes bytes starting at byte `offset` of `path` -- offset = 3 + S*mbytes for a PLINK .bed
 * (data.cpp:215).  The magic bytes are skipped, not validated, as in the reference. */
int gv_upload_bed_file(gv_ctx* ctx, const char* path, int64_t offset);
/* Synthetic shard generated on the device (bench / tests; SURVEY 8d recipe with an integer hash so that
 * gvamp_amd.synth.synth_bed() reproduces it bit for bit on the host).  miss_ppm: missing rate in 1e-6. */
int gv_synth_bed(gv_ctx* ctx, uint64_t seed, uint32_t miss_ppm);
/* The same with linkage disequilibrium: inside every block of ld_block consecutive (global) markers a genotype copies, with
 * probability ld_ppm / 1e6, the block's per-individual latent draw instead of its own -- block-correlated columns, as real
 * genotypes have them (the LMMSE CG then needs tens of steps instead of 4-5).  ld_block = 0: gv_synth_bed. */
int gv_synth_bed_ld(gv_ctx* ctx, uint64_t seed, uint32_t miss_ppm, uint32_t ld_block, uint32_t ld_ppm);
/* ---- methylation data: `data` with type_data == "meth" (data.cpp:54-57, :107-110) --------------------------------------
 * A dense fp64 design matrix: M*N doubles, marker-major (meth_data[i*N + j], read_methylation_data data.cpp:241-278), kept resident
 * in HBM with the row pitch padded to a multiple of 64 doubles (zeros in the padding).  Uploading either kind -- bed or meth --
 * replaces the dataset held before; gv_get_layout returns 3 while a dense matrix is resident.  The dataset kind is dispatched
 * ahead of the kernel mode and the layout: gv_set_kernel_mode / gv_set_layout are ignored for dense data (fp64 VALU kernels
 * of their own, decomposition derived from N, M and the CU count, bit-reproducible), and the solvers take the host-driven CG loops.
 *   gv_marker_stats : mave = sum x na / nonas, msig = 1 / sqrt(sum ((x - mave) na)^2 / (nonas - 1)) raised to alpha_scale as the
 *                     reference does (data.cpp:487-540); a constant column gets msig = 1.
 *   gv_atx          : out[m] = msig[m] sum_{j<N} (x[m][j] - mave[m]) p[j] / sqrt(N) (data.cpp:783-797, :814-835), p used as given
 *                     at every individual (no phenotype mask, as the meth dot_product; bed data: p is masked on its way in).
 *   gv_ax           : out[j] = sum_i (x[i][j] - mave[i]) msig[i] v[i] / sqrt(N) (data.cpp:1013-1045), exact zeros at the pad slots
 *                     j >= N.  The phenotype mask is NOT applied: the reference's meth Ax leaves individuals with a missing
 *                     phenotype unmasked, and so does this one (bed data: masked, as data.cpp:972 does).
 *   two-vector forms: one read of the matrix for both vectors; each slot is bit-identical to the one-vector call.
 * Not available for dense data (non-zero return, the message names the reason): gv_download_bed; gv_people_stats and the N-space
 * solvers gv_cg_solve_aat* (the reference's meth branch of compute_people_statistics, data.cpp:633-672, never reduces or
 * finalises its sums); gv_pvals_* (its meth branch of pvals_calc, data.cpp:1187-1223, computes and stores nothing);
 * gv_set_decomp (nothing to tune). */
/* x: M*N doubles of this shard, marker-major. */
int gv_upload_meth(gv_ctx* ctx, const double* x, size_t n);
/* The same from a file of doubles: M*N of them starting at byte `offset` of `path` -- offset = S*N*8 (data.cpp:259) -- streamed
 * through bounded pinned buffers (host memory stays O(64 MB) however large the shard). */
int gv_upload_meth_file(gv_ctx* ctx, const char* path, int64_t offset);
/* Synthetic methylation matrix generated on the device: value(g, n) = c_g 2^-12 + (u0 + u1 + u2 + u3) 2^-19 for global marker g,
 * an 11-bit per-marker centre c_g and four 16-bit hash fields u_k (an Irwin-Hall sum): every value is exact in fp64, so
 * gvamp_amd.synth.synth_meth(N, M, seed, S) reproduces the matrix bit for bit on the host. */
int gv_synth_meth(gv_ctx* ctx, uint64_t seed);
/* ---- compact dense data: dosages as 8- or 16-bit codes (`data` with type_data == "dosage8" / "dosage16") -----------------------
 * The dense kind above at 1 or 2 bytes per entry: X[m][n] = scale * B[m][n] with B unsigned integer codes, M*N of them, marker-major,
 * resident with the row pitch padded to a multiple of 64 codes (zeros in the padding).  PLINK 2 stores a dosage as a 16-bit code
 * (scale 1/16384); 8-bit codes are the usual compressed form (scale 1/127).  By default every code is a value; missing entries are
 * opt-in per context (gv_set_dosage_missing below: the all-ones code, as PLINK 2 writes it).  Uploading any kind -- bed, meth,
 * dosage -- replaces the dataset held before; gv_get_layout returns 4 (8-bit) or 5 (16-bit) while codes are resident.
 * Semantics are exactly those of the dense fp64 kind: statistics over the individuals with a phenotype, gv_ax applies no mask
 * and writes exact zeros at the pad slots, gv_atx uses p as given, the two-vector forms read the matrix once and each slot is
 * bit-identical to the one-vector call, results are bit-reproducible (no atomics), offsets are 64-bit, kernel mode and layout
 * are ignored.  The statistics are DEFINED in code units (this is the contract, not an implementation detail):
 *   mu'  = (sum_present b) / nonas, the integer sum exact;       mave = scale * mu'
 *   q    = sum_present (b - mu')^2 (second pass);                msig = 1 if q == 0 else (scale * sqrt(q / (nonas - 1)))^-alpha_scale
 * so a constant column has q == 0 and msig = 1 exactly whatever the scale (in value units a non-dyadic scale such as 1/127 hides
 * it behind rounding).  The products form (b - mu') per entry and carry msig * scale in the per-marker weight.
 * Not available (non-zero return, the message names compact dosage data): everything the dense fp64 kind refuses --
 * gv_download_bed, gv_people_stats, gv_cg_solve_aat*, gv_pvals_*, gv_set_decomp -- and gv_set_cg_precond kind 1.
 * The one exception: while gv_set_ld_dosage(ctx, 1) is in force and the resident codes are 8 bits wide, gv_set_cg_precond kind 1 is
 * accepted (the LD-block preconditioner of 8-bit dosage codes, at the end of this header).
 * bits other than 8 or 16 and a scale that is not positive and finite are refused. */
/* codes: M*N codes of this shard, marker-major: uint8_t when bits == 8, uint16_t (host byte order) when bits == 16. */
int gv_upload_dosage(gv_ctx* ctx, const void* codes, size_t n, int bits, double scale);
/* The same from a file: M*N codes starting at byte `offset` of `path` -- offset = S*N*bits/8 -- streamed through the bounded
 * pinned buffers of gv_upload_meth_file; a file that ends early is reported with the marker it ends in. */
int gv_upload_dosage_file(gv_ctx* ctx, const char* path, int64_t offset, int bits, double scale);
/* Synthetic codes generated on the device (scale 1/127 for 8 bits, 1/16384 for 16): per-marker allele frequencies spread over about
 * 0.01-0.5, genotype g in {0, 1, 2} from two allele draws, code = g * 3 * 2^(bits-3) + jitter with jitter < 2^(bits-2): the full
 * code range is used (codes >= 128 / >= 32768 occur).  gvamp_amd.synth.synth_dosage(N, M, seed, bits, S) reproduces it bit for bit. */
int gv_synth_dosage(gv_ctx* ctx, uint64_t seed, int bits);
/* ---- missing entries in compact dosage data (additions only: GV_ABI_VERSION stays 4) -------------------------------------------
 * gv_set_dosage_missing(ctx, 1): the all-ones code -- 255 at 8 bits, 65535 at 16 bits, the code PLINK 2 reserves -- is a MISSING entry.
 * A reserved code, not a mask plane: no extra byte is stored or read.  The setting is read by the next gv_upload_dosage,
 * gv_upload_dosage_file or gv_synth_dosage*; changing it while codes are resident is refused (their statistics would be stale).
 * Default 0: 255 / 65535 are the values they are, and nothing changes by a bit.  Methylation data have no missing code.
 * With the option on let b_kn = 0 where the code of marker k, individual n is the reserved one, 1 otherwise, na_n the phenotype mask.
 * Everything is the definition above with b put where the bed kind has it (data.cpp:951-988, :1155-1176):
 *   cnt_k = sum_n b_kn na_n                          an exact integer (gv_marker_counts)
 *   mu'_k = (sum_n code b na) / cnt_k                the integer sum exact; mu'_k = 0 when cnt_k == 0
 *   q_k   = sum_n ((code - mu'_k) b na)^2            second pass
 *   msig_k = 1 if q_k == 0 else (scale * sqrt(q_k / (nonas - 1)))^-alpha_scale;     mave_k = scale * mu'_k
 *            -- the divisor is the global nonas - 1, not cnt_k - 1, exactly as the bed statistics divide
 *   operator entry = (code - mu'_k) * (msig_k * scale) * b_kn / sqrt(N): formed per entry, never split into two sums; a missing
 *            entry contributes an exact zero to gv_ax, gv_atx and their two-vector forms.
 * The dense rules are unchanged: gv_ax applies no phenotype mask, gv_atx uses p as given, pad slots are exact zeros, each slot of a
 * two-vector call is bit-identical to the one-vector call, no atomics anywhere.
 * gv_assoc_loo / gv_assoc_loco: value_n = (code - mu'_k) * (msig_k * scale) * b_kn * na_n, the LOO self term uses the same value, and
 * the sample size of marker k is cnt_k where it is nonas otherwise; sumy = sum b na p and sumsqy = sum b na p^2 run over the marker's
 * present entries (a marker with cnt_k == nonas takes the pass's totals, which they are).  A marker with cnt_k < 3 or q_k == 0 gives
 * NaN in all four outputs.
 * The summation order of every kernel is that of the plain kernels, so a data set without a reserved code gives the same bits with
 * the option on or off; a shard in which the ingest counted no reserved code therefore runs the plain kernels (gv_dosage_info). */
int gv_set_dosage_missing(gv_ctx* ctx, int on);
/* gv_synth_dosage's generator with missing entries; implies gv_set_dosage_missing(ctx, 1).  The generated code is CLAMPED one below
 * the reserved code (254 / 65534 where gv_synth_dosage emits 255 / 65535); then, per entry, an independent draw -- the high 32 bits of
 * a second hash of the entry below miss_ppm * 2^32 / 10^6 -- replaces it by the reserved code.  miss_ppm <= 1000000.
 * gvamp_amd.synth.synth_dosage_na(N, M, seed, bits, miss_ppm, S) reproduces it bit for bit. */
int gv_synth_dosage_na(gv_ctx* ctx, uint64_t seed, int bits, uint32_t miss_ppm);
/* Block-correlated synthetic codes: gv_synth_dosage's columns are independent, so nothing that exploits LD can be shown on them.
 * Integer only, gv_synth_dosage's constants (hm, base, maf and the entry hash r) and gv_synth_bed_ld's block latent
 * (lbase from the global marker index / ld_block; ld_block >= 1, ld_ppm <= 1000000):
 *   rs = splitmix64(r ^ 0x9FB21C651E98DF25), lat = splitmix64(lbase + n);
 *   the two allele draws read the low 32 bits of lat where rs >> 32 < ld_ppm * 2^32 / 10^6, of r elsewhere; the jitter always comes
 *   from the high 32 bits of r; a code equal to the reserved one is clamped one below it (also with miss_ppm == 0);
 *   where splitmix64(rs ^ 0x2545F4914F6CDD1D) >> 32 < miss_ppm * 2^32 / 10^6 the reserved code replaces the code -- a third hash, so
 *   that missingness is independent of the LD draw.
 * miss_ppm > 0 implies gv_set_dosage_missing(ctx, 1); with miss_ppm == 0 the setting is left as it is (no reserved code is written).
 * gvamp_amd.synth.synth_dosage_ld(N, M, seed, bits, ld_block, ld_ppm, miss_ppm, S) reproduces it bit for bit. */
int gv_synth_dosage_ld(gv_ctx* ctx, uint64_t seed, int bits, uint32_t miss_ppm, uint32_t ld_block, uint32_t ld_ppm);
typedef struct {
    double scale;          /* of the resident codes; 0 when none are resident */
    uint64_t reserved;     /* reserved codes found at the last ingest of this shard: counted on the device behind the copy into the
                            * pitched rows, exact; 0 when the option was off at that ingest (nothing is counted then) */
    int bits;              /* 8 or 16; 0 when no codes are resident */
    int missing;           /* the option the resident codes were uploaded with; without resident codes, the current setting */
    int na_kernels;        /* 1: the missing-aware kernels are in use (option on and reserved != 0, or GV_DOSAGE_NA_KERNELS=1) */
    int pad_;
} gv_dosage_stats;
int gv_dosage_info(gv_ctx* ctx, gv_dosage_stats* out);
/* ---- fixed-point i8 MFMA route for 8-bit dosage codes (additions only: GV_ABI_VERSION stays 4) ------------------------------------
 * gv_set_dosage_route(ctx, route): 0 (default) = the fp64 VALU kernels of the dosage kind, 1 = the products gv_ax / gv_atx, their
 * two-vector forms and everything built on them (gv_lmmse_mult, the CG solvers, the fused solves) run in fixed point on the i8 matrix
 * pipe, on the SAME resident rows (no second copy of the codes).  Any other value is refused.  A request, per context; it may be made
 * before or after an upload and outlives the dataset.  It is IN FORCE only while 8-bit codes are resident and the plain (not the
 * missing-aware) kernels would run (and N <= 2^26: a lane offset of the Ax kernel is 32 bits wide); on 16-bit codes, on a shard with reserved codes under gv_set_dosage_missing, under
 * GV_DOSAGE_NA_KERNELS=1, on bed and on methylation data the request is kept and nothing changes by a bit.  Statistics, gv_assoc_* and
 * the ingest keep their kernels on either route.  gv_get_dosage_route reports both (either pointer may be NULL).
 * Accuracy contract of route 1: that of kernel mode 1 (above) scaled by the code range.  A vector enters a product in fixed point with
 * ONE exponent (|q| < 2^54 relative to its largest entry: per-entry error 2^-55 max|v|), an entry of the matrix is |b - mu'| <= 255
 * codes, everything after the quantisation is exact integer arithmetic with one final rounding.  With the factor-16 slack of mode 1:
 *   Ax : |out[n] - exact[n]| <= M * 2^-50 * (255 * scale / 2) * max_i |msig[i] x[i]| / sqrt(N),
 *   ATx: |out[m] - exact[m]| <= N * 2^-50 * (255 * scale / 2) * msig[m] * max_n |p[n]| / sqrt(N)
 * -- an ABSOLUTE error relative to the vector's largest entry, not relative to each output entry.  The multiplier 2^(54-e) of the
 * quantisation is at most 2^1000: where the largest entry of the quantised vector (p; msig[i] scale x[i] in Ax) is below 2^-946 the
 * per-entry error is 2^-1001 and the bounds hold with that largest entry replaced by 2^-946.  A zero vector gives zeros; one entry
 * that is not finite gives NaN in every output entry of that vector (pad slots of gv_ax stay zero).  Results are bit-reproducible,
 * independent of the work decomposition (every sum is an integer: no order enters), each slot of a two-vector call is bit-identical to
 * the one-vector call, pad slots of gv_ax are exact zeros, no atomics -- but they are not bit-equal to route 0. */
int gv_set_dosage_route(gv_ctx* ctx, int route);
int gv_get_dosage_route(const gv_ctx* ctx, int* requested, int* in_force);
/* cnt: M host doubles, the per-marker counts cnt_k after gv_marker_stats -- nonas for every marker when nothing is missing.
 * Compact dosage data only. */
int gv_marker_counts(gv_ctx* ctx, double* cnt);

/* The PLINK rows back from HBM: only when the raw row layout is resident, i.e. gv_set_layout(ctx, 1, ..) was called before
 * the ingest (not the default). */
int gv_download_bed(gv_ctx* ctx, uint8_t* bed, size_t nbytes);
/* mask4: mbytes nibbles (data.hpp:36; bit k of mask4[j] = individual 4j+k has a phenotype and 4j+k < N);
 * NULL = every individual present (vector-phenotype ctor, data.cpp:86-100).  nonas: data.cpp:100/:150. */
int gv_set_mask(gv_ctx* ctx, const uint8_t* mask4, int64_t nonas);
/* compute_markers_statistics (data.cpp:392-546, scalar-path semantics :451-484). */
int gv_marker_stats(gv_ctx* ctx, double alpha_scale);
int gv_get_marker_stats(gv_ctx* ctx, double* mave, double* msig); /* M doubles each (data.hpp:95-98) */
/* ---- a context is reused: what an input change invalidates, and the call that restores it ------------------------------------------
 * A context may see several masks, alpha_scales, data sets, layouts and dimensions in its life.  After the calls of the right-hand
 * column it answers bit for bit as a context created for the new state (tests/test_gpu_context_reuse.py holds every row to that); an
 * entry point asked BEFORE them refuses with a message naming the missing call -- it never answers from the previous state.
 *
 *   the caller changes                        | goes stale                                            | restored by
 *   ------------------------------------------+-------------------------------------------------------+---------------------------------
 *   gv_set_mask                               | marker statistics (mave, msig, genotype counts, the   | gv_marker_stats
 *                                             | dosage mean codes and per-marker counts), people      | (+ gv_people_stats before an
 *                                             | statistics, window Grams and inverses                 | N-space solve)
 *   gv_marker_stats (a new alpha_scale, or    | people statistics, window Grams and inverses          | gv_people_stats before an N-space
 *   the same one again)                       |                                                       | solve; Grams: rebuilt on demand
 *   gv_upload_* / gv_synth_* (any kind; it    | the data set held before, marker and people           | gv_marker_stats (+ gv_people_stats)
 *   replaces the data set held before)        | statistics, dosage counts, Grams and inverses         |
 *   gv_set_layout                             | nothing until the next bed upload, which builds it    | gv_upload_bed, gv_marker_stats
 *   gv_set_kernel_mode, gv_set_dosage_route   | nothing: read by every product; the marker statistics | -- (people statistics of kernel
 *                                             | are the same exact counts in every kernel family      | mode 0 / 1: gv_people_stats again)
 *   gv_set_ld_dosage, gv_set_cg_precond       | window Grams and inverses (rebuilt on demand)         | --
 *   gv_set_screen_dosage                      | nothing: read by every screen call; no product and no | --
 *                                             | statistic depends on it                               |
 *   gv_set_dosage_missing                     | refused while codes uploaded with the other setting   | gv_set_dims or an upload of another
 *                                             | are resident                                          | kind first, then the upload
 *   gv_set_dims                               | everything above, the mask (everyone present again)   | gv_set_mask, upload, gv_marker_stats;
 *                                             | and EVERY gv_vec of the context                       | gv_vec_free + gv_vec_alloc
 *
 * The N-space solvers gv_cg_solve_aat* refuse until gv_people_stats has run after the LAST gv_marker_stats.  The M-space solvers and
 * every product refuse until gv_marker_stats has run after the last gv_set_mask or upload.
 *
 *   gv_set_mask, gv_marker_stats, gv_upload_* | the covariate side of the adjusted screen (the basis  | gv_marker_stats, then
 *   / gv_synth_*, gv_set_dims                 | Q and the per-marker v of gv_screen_cov_set)          | gv_screen_cov_set
 *
 * gv_screen_cov_dev refuses, naming gv_screen_cov_set, until that call has run after the LAST gv_marker_stats
 * (tests/test_gpu_screen_cov_reuse.py holds this row as the other file holds the rows above).
 * What survives a data set (and gv_set_dims): the options "that outlive the data set" -- kernel mode, layout request, dosage route,
 * gv_set_dosage_missing, gv_set_ld_dosage, gv_set_screen_dosage, the preconditioner kind and window, gv_set_expected_passes, the communicator, timing -- and
 * the ticket counter of the streaming kernels.  The tuner's decomposition picks are made again per resident layout (and change no
 * bit); the run-ahead hints of the device-resident CG go with the data set (they change no bit either).
 * Vectors: a gv_vec belongs to the context that allocated it and to the dimensions it was allocated under.  Every entry point checks
 * each gv_vec argument and refuses, naming the argument, one that belongs to another context or that survived gv_set_dims. */

/* ---- matvecs with the reference's host signatures ---------------------------------------------------
 * data::Ax (data.cpp:848-1009): x[M] -> out[4*mbytes], summed over ranks (if a communicator is attached),
 * masked, scaled by 1/sqrt(N).  data::ATx (data.cpp:810-835): p[4*mbytes] -> out[M], scaled by 1/sqrt(N). */
int gv_ax(gv_ctx* ctx, const double* x, double* out);
int gv_atx(gv_ctx* ctx, const double* p, double* out);

/* Resident HBM layouts built at the next gv_upload_bed / gv_synth_bed: raw_rows = the PLINK rows (pitch-padded;
 * needed by kernel mode 0 and gv_download_bed); stripes selects the re-encoded 2-bit layout of kernel mode 1:
 *   0 none, 1 two stripe sets (marker-major for ATx, individual-major for Ax: 2 x M*N/4 bytes resident),
 *   2 ONE tile layout that serves both products (M*N/4 bytes resident; bit-identical results),
 *   3 auto: the tile layout, unless the caller announced a long run (gv_set_expected_passes >= 1000) and two stripe sets (their
 *     ATx is 2-5 % faster) fit the free HBM at ingest.
 * Default: raw_rows = 0, stripes = 3 -- what bench.py measures and what a binding that never calls this gets (INTEGRATION.md
 * section B): the rows stream through a chunk buffer at ingest and only the re-encoded layout stays resident, so a 100 GB
 * shard occupies 100 GB (or 200 GB) of HBM, not 300.  raw_rows = 1 is needed by kernel mode 0 and gv_download_bed only. */
int gv_set_layout(gv_ctx* ctx, int raw_rows, int stripes);
int gv_get_layout(const gv_ctx* ctx);   /* resident now: 0 none, 1 two stripe sets, 2 tile layout, 3 dense fp64 matrix (meth),
                                         * 4 / 5 dense 8- / 16-bit dosage codes */
/* kernel family for Ax/ATx: 1 (default) = i8 MFMA fixed-point kernels on the re-encoded layout (0.8 of the HBM roofline,
 * results within 2e-14 of fp64 sums, bit-reproducible); 0 = fp64 VALU kernels on the raw rows (parity anchor, 4-9 % of the
 * roofline; needs gv_set_layout(ctx, 1, ..) before ingest); 2 = two-level fixed point on the re-encoded layout (below). */
/* Accuracy contract of kernel mode 1.  A vector enters a product in fixed point with ONE exponent for the whole vector
 * (|q| < 2^54 relative to its largest entry); the product itself is exact integer arithmetic with one final rounding (the integer
 * sum to fp64: as fl(fl(hi) 2^32 + fl(lo)), which is ONE rounding while |lo| <= 2^53 -- any vector up to N = 2 088 960 individuals /
 * M = 1 044 480 markers of a shard, and all but adversarial vectors beyond), followed by the few fixed roundings of the epilogue
 * (mean correction, msig, 1/sqrt(N)); DESIGN.md section 4 lists the sequence, tests/bed_fixed_restatement.py restates it.  Hence
 *   Ax : |out[n] - exact[n]| <= M * 2^-50 * max_i |msig[i] x[i]| / sqrt(N),
 *   ATx: |out[m] - exact[m]| <= N * 2^-50 * msig[m] * max_n |p[n]| / sqrt(N)
 * (worst case; typical errors are sqrt(M) resp. sqrt(N) times smaller), i.e. an ABSOLUTE error relative to the vector's largest
 * entry -- below the error of fp64 summation in relative l2 (measured <= 2e-14 against the fp64 oracle over 60 decades of overall
 * scale), but not relative to each output entry: an entry more than 2^54 below the vector's maximum is flushed to zero, and an
 * output that does not see the large entries (Ax at an individual whose genotype is MISSING at the one marker carrying a huge
 * effect) is accurate to the bound above, not to its own last bits as the reference's fp64 sums are there.  The vectors of a VAMP
 * run span a few decades and never come near this; input with more than ~2^40 of dynamic range that needs per-entry relative
 * accuracy should use kernel mode 2 (below).  tests/test_gpu_matvec.py asserts both bounds on such input.
 * Kernel mode 2 (ABI 4) = the fast remedy: TWO-LEVEL fixed point on the same resident layout.  The vector is quantised as in mode 1
 * (the head), the exact fp64 residual v - head is quantised once more with the exponent 54 below (v = head + residual to within
 * 2^-109 of the largest entry: ~108 bits instead of 54), and head and residual travel as the two slots of ONE two-vector pass; the
 * planes of that pass give a missing genotype an exact zero (a' = a if present else 0; b = present), as the reference's table does
 * (data.cpp:951-988), instead of "3 c + (mave - 3) c - mave c", which cancels only to rounding.  An output entry that does not see
 * the huge entries is then accurate to its own magnitude (the adversarial case above: 1e-9 ... 1e-3 relative in mode 1, < 1e-12 in
 * mode 2) for up to ~2^55 of in-vector dynamic range.  Cost: one two-vector pass per product (1.0-1.1 x a one-vector pass); the
 * two-vector entry points run two such passes; the solvers take the host-driven loops (the device-resident CG and GV_OVERLAP are
 * mode-1 machinery); marker / people statistics and p-values are those of mode 1 (exact counts; their sums are not affected).
 * Results are bit-reproducible and independent of layout and decomposition, as in mode 1 -- but not bit-equal to mode 1. */
int gv_set_kernel_mode(gv_ctx* ctx, int mode);
int gv_get_kernel_mode(const gv_ctx* ctx);

/* ---- device-resident vectors (the std::vector<double> temporaries of vamp.cpp live here) ------------ */
enum { GV_SPACE_M = 0, GV_SPACE_N = 1 }; /* length M, or length 4*mbytes (padded internally) */
int gv_vec_alloc(gv_ctx* ctx, int space, gv_vec** out);
void gv_vec_free(gv_ctx* ctx, gv_vec* v);
int64_t gv_vec_len(const gv_vec* v); /* logical length: M or 4*mbytes */
int gv_vec_upload(gv_ctx* ctx, gv_vec* v, const double* src);
int gv_vec_download(gv_ctx* ctx, const gv_vec* v, double* dst);
int gv_vec_fill(gv_ctx* ctx, gv_vec* v, double value);
int gv_vec_copy(gv_ctx* ctx, gv_vec* dst, const gv_vec* src);
/* out = a*x + b*y (y may be NULL when b == 0; out may alias x or y) */
int gv_vec_axpby(gv_ctx* ctx, gv_vec* out, double a, const gv_vec* x, double b, const gv_vec* y);
/* out = x .* y element-wise (out may alias x or y): the freeze mask of vamp.cpp:308,:353 applied on the device */
int gv_vec_mul(gv_ctx* ctx, gv_vec* out, const gv_vec* x, const gv_vec* y);
/* inner_prod (utilities.cpp:190-210): sync != 0 adds the cross-rank all-reduce of the scalar. */
int gv_vec_dot(gv_ctx* ctx, const gv_vec* x, const gv_vec* y, int sync, double* out);
/* several dots in one pass and ONE all-reduce: out[k] = <x[k], y[k]> */
int gv_vec_dots(gv_ctx* ctx, int n, const gv_vec* const* x, const gv_vec* const* y, int sync, double* out);
/* The scalars one VAMP iteration reads after its solves (vamp.cpp:631, :686-693, :892-927, :741-749, :1295-1317), in one launch
 * and one read-back: out[k] = <xa - xb, ya - yb> (xb / yb may be NULL: the plain vector); pairs of either space may be mixed;
 * sync != 0 adds the cross-rank all-reduce of that scalar.  Each scalar is bit-identical to gv_vec_axpby(t, 1, xa, -1, xb) ...
 * gv_vec_dot(t, u): the difference is rounded once, the sum runs in the same order. */
typedef struct gv_dot_spec {
    const gv_vec* xa; const gv_vec* xb;
    const gv_vec* ya; const gv_vec* yb;
    int sync;
} gv_dot_spec;
int gv_vec_dots_ex(gv_ctx* ctx, int n, const gv_dot_spec* spec, double* out);
int gv_ax_dev(gv_ctx* ctx, const gv_vec* x, gv_vec* out);  /* data::Ax on handles */
int gv_atx_dev(gv_ctx* ctx, const gv_vec* p, gv_vec* out); /* data::ATx on handles */
/* Two vectors per pass over the shard (kernel mode 1; two single passes otherwise): outa = A xa, outb = A xb, and
 * outa = A^T pa, outb = A^T pb.  Results are bit-identical to the one-vector calls (exact integer accumulation). */
int gv_ax2_dev(gv_ctx* ctx, const gv_vec* xa, const gv_vec* xb, gv_vec* outa, gv_vec* outb);
int gv_atx2_dev(gv_ctx* ctx, const gv_vec* pa, const gv_vec* pb, gv_vec* outa, gv_vec* outb);
/* phenotype y (length N) -> N-space handle with NA / pad slots zeroed: data::filter_pheno (data.cpp:1065-1079) */
int gv_set_phen(gv_ctx* ctx, gv_vec* y_out, const double* y_host);

/* ---- solver: vamp::lmmse_mult (vamp.cpp:1074-1118), vamp::precondCG_solver (vamp.cpp:1130-1229) ------ */
int gv_lmmse_mult(gv_ctx* ctx, const gv_vec* v, double tau, double gam2, gv_vec* out);
typedef struct {
    int iters;           /* CG steps executed */
    int converged;       /* 1 if a stopping rule fired before max_iter */
    double rel_res;      /* ||r|| / ||v|| at exit (vamp.cpp:1215) */
    double onsager;      /* gam2 * <v, mu> at exit (denoiser == 0 only, vamp.cpp:1176) */
    int n_ax, n_atx;     /* matvec calls made */
    int n_relres;        /* entries written to relres (an Onsager-rule exit skips the last residual update) */
} gv_cg_stats;
/* mu_start may be NULL (zeros).  denoiser: 1 = LMMSE solve, 0 = Onsager probe solve (extra stopping rule).
 * relres (may be NULL): max_iter doubles receiving ||r||/||v|| after every step. */
int gv_cg_solve(gv_ctx* ctx, const gv_vec* v, const gv_vec* mu_start, double tau, double gam2, int denoiser,
                int max_iter, gv_vec* mu_out, gv_cg_stats* stats, double* relres);

/* The LMMSE solve (v_a, optional warm start, denoiser = 1 rules) and the Onsager probe solve (v_b, zero start, denoiser = 0
 * rules) of one VAMP iteration run in lock-step on the shared operator (tau, gam2): every round applies the operator to
 * the pending direction of each still-active solve in ONE two-vector Ax + ATx pair.  Per solve the iterates, stopping
 * rules and results are those of gv_cg_solve. */
int gv_cg_solve2(gv_ctx* ctx, const gv_vec* v_a, const gv_vec* mu_start_a, const gv_vec* v_b, double tau, double gam2,
                 int max_iter, gv_vec* mu_a, gv_vec* mu_b, gv_cg_stats* stats_a, gv_cg_stats* stats_b,
                 double* relres_a, double* relres_b);

/* gv_cg_solve2 plus by-products that cost no further pass over the shard.  Every member may be NULL (= not wanted):
 *   ride_x / ride_out : ride_out = data::Ax(ride_x) (data.cpp:848) for an M-vector unrelated to the solves -- e.g.
 *                       z1 = A x1_hat of vamp.cpp:429 -- computed in the free slot of the first round in which only one
 *                       solve is still active (a two-vector pass costs what a one-vector pass costs), else by one pass of
 *                       its own after the solves.  Bit-identical to gv_ax_dev.
 *   a_mu_a   (N-space): A mu_a, accumulated from the products A p_k that CG forms anyway
 *                       (A mu_a = A mu_start + sum_k alpha_k A p_k): the A x2_hat of vamp.cpp:897 without its Ax.
 *   ata_mu_b (M-space): A^T A mu_b = (v_b - r_b - gam2 mu_b) / tau from the final residual of solve b: the
 *                       A^T (A invQ u) of vamp.cpp:913-914 without its Ax and ATx.
 * a_mu_a and ata_mu_b are algebraic identities of the CG recurrences: they agree with the explicit products to rounding
 * (~1e-13 relative), not bit for bit. */
typedef struct gv_cg_extras {
    const gv_vec* ride_x;
    gv_vec* ride_out;
    gv_vec* a_mu_a;
    gv_vec* ata_mu_b;
} gv_cg_extras;
int gv_cg_solve2x(gv_ctx* ctx, const gv_vec* v_a, const gv_vec* mu_start_a, const gv_vec* v_b, double tau, double gam2,
                  int max_iter, gv_vec* mu_a, gv_vec* mu_b, gv_cg_stats* stats_a, gv_cg_stats* stats_b,
                  double* relres_a, double* relres_b, const gv_cg_extras* extras);
/* gv_cg_solve2x whose warm start costs no pass.  precondCG_solver opens with r = v - Q mu_start (vamp.cpp:1142-1145: one Ax
 * and one ATx); when mu_start_a is the mu_a of the PREVIOUS call, that call's final residual already holds the product:
 * Q' mu = v' - r'  =>  A^T A mu = (v' - r' - gam2' mu) / tau'.  Every member may be NULL:
 *   ata_mu_a       (M-space, out): A^T A mu_a of THIS solve from its final residual -- hand it to the next call;
 *   ata_mu_start_a (M-space, in) : A^T A mu_start_a (the previous call's ata_mu_a; may be the same handle as ata_mu_a).
 *                                  r = v_a - tau * ata_mu_start_a - gam2 * mu_start_a replaces the operator application;
 *   a_mu_start_a   (N-space, in) : A mu_start_a, required with ata_mu_start_a when extras->a_mu_a is wanted (its
 *                                  accumulation starts there; may be the same handle as extras->a_mu_a, i.e. the previous
 *                                  call's a_mu_a left in place).
 * An identity of the CG recurrences like a_mu_a / ata_mu_b: equal to the explicit products to rounding, not bit for bit;
 * the rounding of successive calls adds up (no call re-anchors on an explicit product), ~1e-16 relative per CG step. */
typedef struct gv_cg_warm {
    const gv_vec* ata_mu_start_a;
    const gv_vec* a_mu_start_a;
    gv_vec* ata_mu_a;
    /* Solve b starts from zero, so its first step applies the operator to v_b / diag.  When v_b is the same vector call after call
     * (the Onsager probe of vamp.cpp:875 is re-seeded identically every iteration), A^T A v_b never changes:
     *   ata_v_b (M-space): with have_ata_v_b == 0 an OUTPUT -- A^T A v_b, taken from solve b's first application (written when
     *                      max_iter > 0); with have_ata_v_b != 0 an INPUT -- that first application becomes
     *                      (tau / diag) * ata_v_b + gam2 * v_b / diag and costs no pass, so solve b is one pass pair shorter.
     * The caller owns the invariant "same v_b as when ata_v_b was written".  Equal to the explicit product to rounding.
     * Refused under the LD preconditioner (gv_set_cg_precond kind 1): its first step applies the operator to M^-1 v_b, no multiple
     * of v_b, so there is nothing to capture or use -- pass NULL there. */
    gv_vec* ata_v_b;
    int have_ata_v_b;
} gv_cg_warm;
int gv_cg_solve2w(gv_ctx* ctx, const gv_vec* v_a, const gv_vec* mu_start_a, const gv_vec* v_b, double tau, double gam2,
                  int max_iter, gv_vec* mu_a, gv_vec* mu_b, gv_cg_stats* stats_a, gv_cg_stats* stats_b,
                  double* relres_a, double* relres_b, const gv_cg_extras* extras, const gv_cg_warm* warm);

/* ---- denoiser side (fused element-wise kernels) ------------------------------------------------------
 * vamp::g1 / g1d over a vector (vamp.cpp:805-869; loops :292-310): x1 = g1(r1), sums[0] = sum g1d(r1) (local),
 * sums[1] = sum (x1-r1)^2 (local).  vars already multiplied by N (vamp.cpp:154-155).  d_out may be NULL. */
int gv_denoise(gv_ctx* ctx, const gv_vec* r1, double gam1, const double* probs, const double* vars, int L,
               gv_vec* x1_out, gv_vec* d_out, double* sums2);
/* one E-step of vamp::updatePrior (vamp.cpp:953-1013): sums[0] = sum_i pi_i, sums[1+2j] = sum_i beta_ij pi_i,
 * sums[2+2j] = sum_i beta_ij (m_ij^2 + v_j) pi_i for j = 0..L-2 (local sums; caller all-reduces 1+2(L-1)). */
/* The same two with their sums taken over the ranks (the MPI_Allreduce of vamp.cpp:313 / :326 and of :990 / :1012-1013 folded in):
 * the device buffer is all-reduced in stream before the one read-back, where gv_denoise + gv_allreduce_host make a second round trip
 * (host -> device -> all-reduce -> host) per call -- about seven per VAMP iteration on a sharded job.  One rank: identical to the
 * local forms. */
int gv_denoise_global(gv_ctx* ctx, const gv_vec* r1, double gam1, const double* probs, const double* vars, int L,
                      gv_vec* x1_out, gv_vec* d_out, double* sums2);
int gv_prior_estep_global(gv_ctx* ctx, const gv_vec* r1, double gam1, double lambda, const double* omegas,
                          const double* vars, int L, double* sums);
int gv_prior_estep(gv_ctx* ctx, const gv_vec* r1, double gam1, double lambda, const double* omegas,
                   const double* vars, int L, double* sums);
/* ---- --model bin_class (vamp_probit.cpp): the z-side probit denoiser over the N individuals ------------------------
 * vamp::g1_bin_class / g1d_bin_class (vamp_probit.cpp:661-705; loops :335-352) with m_cov = 0: z1 = E[z | y, cavity
 * N(p1, 1/tau1)], sums2[0] = sum_n g1d_bin_class, sums2[1] = sum_n (z1 - p1)^2.  y holds 0 / 1 (N-space handle). */
int gv_probit_denoise(gv_ctx* ctx, const gv_vec* p1, const gv_vec* y, double tau1, double probit_var, gv_vec* z1_out,
                      double* sums2);
/* the same with covariates (--C > 0): m_cov[i] = <Z[i], cov_eff> (vamp_probit.cpp:347,:364) shifts the argument of the
 * probit likelihood, c = (p1 + m_cov) / sqrt(probit_var + 1/tau1).  m_cov: N-space handle or NULL. */
int gv_probit_denoise_cov(gv_ctx* ctx, const gv_vec* p1, const gv_vec* y, const gv_vec* m_cov, double tau1,
                          double probit_var, gv_vec* z1_out, double* sums2);

/* ---- --model robust (vamp_Huber.cpp): the z side of Huber-loss VAMP over the N individuals -----------------------------
 * gv_huber_denoise: z1 = g1_Huber(p1, tau1, deltaH, y) (vamp_Huber.cpp:443-461); sums2[0] = sum_n dz1/dp1 (1/(1+1/tau1) where
 * |y - p1| <= (1+1/tau1) deltaH, else 1: the derivative of g1_Huber, which g1d_Huber_der :485-503 is not), sums2[1] =
 * sum_n (z1 - p1)^2.  Pad slots of z1 are written 0.
 * gv_huber_delta: obj_out[g] = (1/N) sum_n E[rho_{grid[g]}(y_n - z)], z ~ N(p1_n, 1/tau1), in closed form, + log Z(grid[g]) with
 * Z(d) = sqrt(2 pi)(2 Phi(d) - 1) + (2/d) exp(-d^2/2): the expected negative log-likelihood of the Huber density, the objective
 * that M_deltaH_update (:554-573) estimates by Monte Carlo without log Z.  1 <= G <= 16, grid values > 0.
 * Both take N-space handles (every rank holds all N: no collective) and give the same bits on every call.
 * vamp::infere_robust (--model robust) calls both every iteration. */
int gv_huber_denoise(gv_ctx* ctx, const gv_vec* p1, const gv_vec* y, double tau1, double deltaH, gv_vec* z1_out,
                     double* sums2);
int gv_huber_delta(gv_ctx* ctx, const gv_vec* p1, const gv_vec* y, double tau1, const double* grid, int G, double* obj_out);

/* ---- --use-XXT-denoiser 1 (vamp.cpp:169-170, :599-606; denoiserXXT.cpp): LMMSE through CG in N-space, matrix-free --
 * data::compute_people_statistics (data.cpp:558-716): per-individual mean, inverse std and count of the standardised
 * genotypes, all-reduced over ranks; kept on the device for gv_cg_solve_aat.  Host copies (4*mbytes doubles each) are
 * optional (NULL).  Kernel mode 0: three fp64 passes over the raw rows.  Kernel mode 1 (or no raw rows resident): four
 * exact fixed-point passes over stripes_n, the quadratic one on the a^2 plane of the 2-bit codes. */
int gv_people_stats(gv_ctx* ctx, double* mave_people, double* msig_people, double* numb_people);
/* vamp::CG_solverAAT (denoiserXXT.cpp:52-130): solves (tau A A^T + gam2 I) mu = v in N-space with the per-individual
 * diagonal preconditioner, stopping at ||r||/||v|| < 1e-4.  mu_start may be NULL (zeros). */
int gv_cg_solve_aat(gv_ctx* ctx, const gv_vec* v, const gv_vec* mu_start, double tau, double gam2, int max_iter,
                    gv_vec* mu_out, gv_cg_stats* stats, double* relres);
/* The N-space solve above (system a: v_a, mu_start_a, N-space) and the Onsager probe solve of the same iteration (system
 * b: gv_cg_solve with denoiser = 0 from a zero start, M-space; vamp.cpp:631 in the --use-XXT-denoiser branch) on shared
 * passes: Q_a = tau A A^T + gam2 I is an ATx followed by an Ax, Q_b = tau A^T A + gam2 I an Ax followed by an ATx, so run
 * half an application out of phase every pass over the shard (after the first) serves both through the two-vector kernels.
 * Per solve the iterates, stopping rules and results are those of the stand-alone calls (bit-identical).
 *   at_mu_a (M-space)           : A^T mu_a, the ATx of denoiserXXT.cpp:47-49 (x2_hat = r2 + gamw A^T mu_a), taken along too;
 *   aat_mu_a (N-space, or NULL) : A A^T mu_a = (v_a - r_a - gam2 mu_a) / tau from the final residual of solve a;
 *   ata_mu_b (M-space, or NULL) : A^T A mu_b likewise (gv_cg_extras) -- identities of the recurrences, equal to rounding. */
int gv_cg_solve_aat2(gv_ctx* ctx, const gv_vec* v_a, const gv_vec* mu_start_a, const gv_vec* v_b, double tau, double gam2,
                     int max_iter, gv_vec* mu_a, gv_vec* at_mu_a, gv_vec* mu_b, gv_cg_stats* stats_a, gv_cg_stats* stats_b,
                     double* relres_a, double* relres_b, gv_vec* aat_mu_a, gv_vec* ata_mu_b);
/* The same with products the caller already holds.  Every member may be NULL / 0:
 *   aat_mu_start_a (N-space): A A^T mu_start_a as the previous call left it in aat_mu_a (may be that very handle);
 *                             r = v_a - tau * aat_mu_start_a - gam2 * mu_start_a then replaces the ATx + Ax pair that opens a
 *                             warm-started CG_solverAAT (denoiserXXT.cpp:76-78);
 *   accumulate_at_mu_a      : at_mu_a = A^T mu_a is accumulated from the A^T p_k every operator application starts with
 *                             (A^T mu_a = A^T mu_start_a + sum_k alpha_k A^T p_k) instead of by a closing ATx pass;
 *   at_mu_start_a (M-space) : A^T mu_start_a for that sum (the previous call's at_mu_a; may be the same handle as at_mu_a) --
 *                             required when aat_mu_start_a skips the opening application, taken from that application otherwise,
 *                             0 for a zero start.
 * Identities of the recurrences: equal to the explicit products to rounding, not bit for bit. */
typedef struct gv_aat_warm {
    const gv_vec* aat_mu_start_a;
    const gv_vec* at_mu_start_a;
    int accumulate_at_mu_a;
    gv_vec* ata_v_b;            /* as in gv_cg_warm: A^T A v_b of the zero-started M-space solve b, captured or handed in */
    int have_ata_v_b;
    /* pre_x / pre_out: the right-hand side of solve a is completed inside the call -- pre_out = A pre_x, then v_a <- v_a - pre_out
     * (v_a is an in/out argument of gv_cg_solve_aat2w for this reason): v = y - A r2 of denoiserXXT.cpp:40-42 with v_a = y, pre_x = r2.
     * That Ax shares its pass with the first half-application of solve b, which puts the two solves in phase from the start
     * (one pass fewer than forming v_a outside).  ride_x / ride_out: ride_out = A ride_x for an M-vector unrelated to the solves
     * (z1 = A x1_hat, vamp.cpp:429), taken in an Ax pass that has a slot free, else by a pass of its own at the end. */
    const gv_vec* pre_x;
    gv_vec* pre_out;
    const gv_vec* ride_x;
    gv_vec* ride_out;
    /* v_a <- v_a - pre_scale * pre_out (0 = 1).  With pre_x = x1_hat, pre_out = z1 and the caller's v_a = y + (gam1/gam2) A r1 the solve
     * gets its right-hand side y - A r2 from A r2 = (eta1/gam2) A x1_hat - (gam1/gam2) A r1 (r2 is that combination, vamp.cpp:485-486)
     * and the iteration's z1 = A x1_hat (vamp.cpp:429) for free: no pass for A r2 (host/vamp.cpp keeps A r1 up to date from A x2_hat). */
    double pre_scale;
} gv_aat_warm;
/* v_a: read only, unless warm->pre_x is set -- then it is updated in place (see pre_x above). */
int gv_cg_solve_aat2w(gv_ctx* ctx, gv_vec* v_a, const gv_vec* mu_start_a, const gv_vec* v_b, double tau, double gam2,
                      int max_iter, gv_vec* mu_a, gv_vec* at_mu_a, gv_vec* mu_b, gv_cg_stats* stats_a, gv_cg_stats* stats_b,
                      double* relres_a, double* relres_b, gv_vec* aat_mu_a, gv_vec* ata_mu_b, const gv_aat_warm* warm);

/* ---- association tests after the loop (vamp.cpp:761-776) ------------------------------------------------------
 * data::pvals_calc (data.cpp:1108-1226, one estimator): leave-one-out t-test p-value of every local marker,
 * pvals[M].  z1 = A x1_hat and y (filtered phenotype) are N-space handles, x1_hat the M-space estimate (the
 * sqrt(N)-scaled x1_hat of vamp.cpp, as passed at :765).  One pass over the genotype shard (two digit vectors, y_mod
 * and y_mod^2, share the 16 MFMA columns) + exact per-marker genotype counts; the regression test and its Student-t tail run in
 * the epilogue of that pass (k_fin_pvals, gv_pval_dev.h), only the p-values cross PCIe. */
int gv_pvals_loo(gv_ctx* ctx, const gv_vec* z1, const gv_vec* y, const gv_vec* x1_hat, double* pvals);
/* data::pvals_calc_LOCO (data.cpp:1235-1353): chrom[M] in 1..23 (read_chromosome_info, data.cpp:346-380); per
 * chromosome one Ax (with its cross-rank all-reduce) + one marker pass.  Markers of other chromosomes get 0. */
int gv_pvals_loco(gv_ctx* ctx, const gv_vec* z1, const gv_vec* y, const gv_vec* x1_hat, const int* chrom,
                  double* pvals);
/* The same, also returning the per-chromosome genetic predictors the reference dumps as <file>_LOCO_chr_<ch>.csv
 * (data.cpp:1276-1281): chrom_pred[(ch-1) * 4*mbytes + n] = (A x1_hat restricted to chromosome ch)[n], summed over ranks,
 * ch = 1..23 (zeros for a chromosome no rank holds).  chrom_pred: 23 * 4*mbytes host doubles, or NULL. */
int gv_pvals_loco_pred(gv_ctx* ctx, const gv_vec* z1, const gv_vec* y, const gv_vec* x1_hat, const int* chrom,
                       double* pvals, double* chrom_pred);

/* ---- the whole association test: effect, standard error, t and p (additions only: GV_ABI_VERSION stays 4) ----------------------
 * gv_pvals_* above return a p-value alone (the reference leaves beta commented out in linear_reg1d_pvals) and refuse the dense
 * kinds.  gv_assoc_* return the full result of the same test, for bed data in both kernel families and for compact dosage data
 * of both widths.  Per local marker k and individual n
 *     value_n = (x_kn - mave_k) * msig_k * b_kn * na_n
 *   bed data    : x = a (0, 1, 2), b = 1 where the genotype is present (data.cpp:1155-1175);
 *   dosage data : x = scale * code, formed in code units as (code - mu'_k) * (msig_k * scale); b == 1, or with
 *                 gv_set_dosage_missing b = 0 at the reserved code.
 * p is the phenotype residual of pvals_calc / pvals_calc_LOCO, zero at NA and pad slots whatever the caller left in y there:
 *   leave-one-out            : y - z1 + value * x1_hat[k] / sqrt(N)
 *   leave-one-chromosome-out : y - z1 + (A x1_hat restricted to the marker's chromosome).
 * With sumx = sum value, sumsqx = sum value^2, sumxy = sum value p, sumy = sum b na p, sumsqy = sum b na p^2, n = sum b na
 * (data.cpp:1164-1176) and s2x, s2y, sxy, rxy as in utilities.cpp:323-326:
 *   beta = sxy / s2x                       effect per unit of the STANDARDISED column; beta * msig_k is the effect per unit of
 *                                          genotype (bed) or dosage value (dosage data)
 *   t    = rxy * sqrt((n - 2) / (1 - rxy^2)), signed
 *   se   = beta / t, evaluated as sqrt((n - 1) / (n - 2) * s2y * (1 - rxy^2) / ((n - 1) * s2x)): t == 0 gives no 0/0
 *   p    = two-sided Student-t tail of |t| with n - 2 degrees of freedom -- for bed data bit-identical to gv_pvals_*.
 * Dosage data: n = nonas for every marker (cnt_k with gv_set_dosage_missing); a constant column (q == 0, msig = 1, value == 0) yields NaN in all four outputs, as a
 * monomorphic bed marker does.  Bed and dosage data alike: a marker with n < 3 -- fewer than three present genotypes or entries among
 * the individuals with a phenotype -- has no degree of freedom left and yields NaN in all four outputs (gv_pvals_* give NaN there
 * too), in every kernel family; so does a bed marker that is monomorphic among its present genotypes.  The sums of a row are formed in a fixed order that depends neither on the call (LOO / LOCO) nor
 * on the other rows of the pass: results are bit-reproducible, and LOCO with x1_hat == 0 on one chromosome equals LOO bit for bit.
 * LOCO: markers whose chromosome is outside 1..23 get 0 in all four outputs; a pass streams the rows of its chromosome only, so the
 * 23 passes read a dosage matrix once.  Vector spaces and marker statistics are checked as gv_pvals_* check them.
 * Not available for methylation data (dense fp64 matrix; non-zero return, the message names methylation data): no test is
 * defined for it. */
typedef struct { double *beta, *se, *t, *p; } gv_assoc_out;   /* each M host doubles, or NULL: that output is not copied out */
int gv_assoc_loo(gv_ctx* ctx, const gv_vec* z1, const gv_vec* y, const gv_vec* x1_hat, const gv_assoc_out* out);
/* chrom as gv_pvals_loco; chrom_pred as gv_pvals_loco_pred: 23 * 4*mbytes host doubles, or NULL. */
int gv_assoc_loco(gv_ctx* ctx, const gv_vec* z1, const gv_vec* y, const gv_vec* x1_hat, const int* chrom,
                  const gv_assoc_out* out, double* chrom_pred);

/* SUM all-reduce of n host doubles over the attached communicator (identity when none): MPI_Allreduce of
 * scalars in vamp.cpp:313,990,1012-1013 */
int gv_allreduce_host(gv_ctx* ctx, double* buf, int n);

/* ---- communicator: stands in for MPI_COMM_WORLD (data.cpp:928/:995; utilities.cpp:203) ---------------
 * RCCL over xGMI, one process per GPU.  Rank 0 calls gv_comm_unique_id and ships the 128 bytes to the
 * other ranks by any out-of-band channel (bench.py: torch.distributed broadcast). */
int gv_comm_unique_id(void* id128);
/* nranks == 1 with id128 == NULL attaches nothing; with an id a 1-rank RCCL communicator is created (self-test). */
int gv_comm_init(gv_ctx* ctx, int nranks, int rank, const void* id128);
/* In-process communicator for tests: `nranks` contexts of one process (one thread each, any GPUs) that name the same
 * `group` behave like nranks ranks; sums are taken in rank order on the host.  Every collective must be entered by
 * all members concurrently (from different threads). */
int gv_comm_init_local(gv_ctx* ctx, int group, int nranks, int rank);
/* Communicator over a caller-supplied transport: every collective of the context becomes
 *   device -> host copy, fn(user, buf, n) [in-place SUM of n host doubles over the nranks ranks; 0 = ok], host -> device copy.
 * For a host that already owns a communicator -- the reference's MPI_COMM_WORLD (`MPI_Allreduce(MPI_IN_PLACE, buf, n,
 * MPI_DOUBLE, MPI_SUM, ...)`, data.cpp:928) -- and for tests that run the ranks as processes sharing one GPU
 * (torch.distributed gloo).  Slower than RCCL (two PCIe hops per message); the sums must be identical on every rank. */
typedef int (*gv_allreduce_fn)(void* user, double* buf, size_t n);
int gv_comm_init_callback(gv_ctx* ctx, int nranks, int rank, gv_allreduce_fn fn, void* user);
/* One communicator per process: ctx joins the communicator `owner` already holds (RCCL, in-process or callback) instead of
 * building another one -- a process that keeps several `data` objects (main_real --run-mode both: a training and a test set)
 * has ONE MPI_COMM_WORLD in the reference, too.  The communicator lives until the last context sharing it is destroyed; both
 * contexts must be driven from the same host thread (their collectives are issued in program order). */
int gv_comm_share(gv_ctx* ctx, const gv_ctx* owner);
/* Overlap of the N-vector exchange of data::Ax with the decode (kernel mode 1, sharded jobs): tiles > 1 cuts the product into
 * that many chunks of individuals and all-reduces each slice on a side HIP stream while the next chunk decodes; 0 / 1 = one
 * message after the whole pass (default; also set by the environment variable GV_OVERLAP).  Bit-identical results. */
int gv_set_overlap(gv_ctx* ctx, int tiles);
/* TEST HOOK, never part of a production job.  A context of a ONE-rank job takes every branch a sharded job takes -- the N-vector
 * exchange inside data::Ax (data.cpp:928/:995), the packed scalar all-reduces (utilities.cpp:203), k_finalize + all-reduce instead of
 * the one-rank shortcuts of the device-resident CG, the side-stream exchange of gv_set_overlap -- with an exchange that is
 * asynchronous and in-stream like RCCL's (no host synchronisation, unlike the gv_comm_init_local / _callback transports):
 *   transport 1: loop-back kernels -- the message moves to scratch, the buffer is filled with NaNs, (delay_us later) it moves back;
 *                a consumer that is not stream-ordered behind its exchange reads NaNs;
 *   transport 2: ncclAllReduce on a 1-rank RCCL communicator (created here if the context holds none);   3: both, RCCL first;
 *   transport 0: back to the plain one-rank paths;   + 4: fault injection -- the overlapped exchange drops its closing event edge
 *                (the harness must then SEE wrong results: tests/test_gpu_forced_multi.py checks that it has teeth).
 * Sums over one rank are the identity, so every result must equal the plain one-rank run BIT FOR BIT (tests/test_gpu_forced_multi.py).
 * Also: environment variable GVAMP_FORCE_MULTI=<transport>[:<delay_us>] at gv_create (drivers, bench.py). */
int gv_debug_force_multi(gv_ctx* ctx, int transport, int delay_us);
int gv_comm_rank(const gv_ctx* ctx);
/* One process per GPU on a multi-socket node: restricts the calling thread -- and every thread it starts afterwards -- to the
 * CPUs of the NUMA node `device` hangs off (sysfs: the PCI device's numa_node, the node's cpulist), intersected with the CPUs it
 * may already use.  *numa_node_out (may be NULL) = that node, or -1 when nothing was changed (single-node host, topology hidden,
 * fewer than 8 CPUs in common, GVAMP_NUMA_BIND=0).  Call it before the first gv_create of the process; the drivers and bench.py do. */
int gv_bind_host_numa(int device, int* numa_node_out);
int gv_comm_size(const gv_ctx* ctx);

/* ---- instrumentation ---------------------------------------------------------------------------------- */
typedef struct {
    int64_t n_ax, n_atx;          /* kernel launches of each matvec since the last reset */
    double ms_ax, ms_atx;         /* HIP-event time spent in them (on the context's stream) */
    double ms_allreduce;          /* HIP-event time of the N-vector all-reduces */
    int64_t n_ax_kernel, n_atx_kernel;   /* timing == 2: launches of the dominant matvec kernel measured ... */
    double ms_ax_kernel, ms_atx_kernel;  /* ... and their summed HIP-event durations */
    int64_t n_ax_pass, n_atx_pass;       /* passes over the genotype shard (a two-vector product counts 2 in n_ax / n_atx
                                          * and 1 here) */
    int64_t n_allreduce;                 /* N-vector exchange steps timed into ms_allreduce (timing 1 or 2; sharded jobs) */
} gv_counters;
/* timing: 0 off; 1 brackets every whole matvec (prep + kernel + epilogue) with HIP events and synchronises per
 * call (development); 2 records event pairs around the dominant matvec kernel only, WITHOUT synchronising --
 * they are resolved in gv_get_counters (live roofline measurement inside a timed region). */
int gv_set_timing(gv_ctx* ctx, int timing);
int gv_get_counters(gv_ctx* ctx, gv_counters* out);
int gv_reset_counters(gv_ctx* ctx);
/* The work decomposition of the four streaming-kernel classes (0 ATx, 1 two-vector ATx, 2 Ax, 3 two-vector Ax) as
 * picked by the on-device tuning (or its cache / an override): what a bench line reports per rank. */
typedef struct {
    int ks;                  /* uniform K-split: segments per group of four row groups */
    int64_t balanced_cells;  /* > 0: balanced decomposition, cells per workgroup (ks unused) */
    int prio;                /* progress-based wave priority on */
    float taper;             /* uniform split: taper of the segment lengths */
    int tuned;               /* 1 once the pick has been made (measured or read from the cache) */
    int64_t whole_quads;     /* balanced only, > 0: hybrid -- that many groups of four row groups go one per workgroup over the
                              * whole K range, only the remaining ones are cut into ranges of balanced_cells cells */
    float geo;               /* uniform split, 0 < geo < 1: segment j is geo^j times segment 0 (big first; replaces taper) */
    int wgs_per_cu;          /* ABI 4: workgroups of the streaming kernel a CU holds: 3 (what the registers allow; 0 on input means
                              * this) or 2 (the launch reserves LDS to that end: faster on some 12.5 GB shapes, slower at 100 GB) */
    float xcd_skew;          /* ABI 4, uniform split with ks >= 2: segments whose workgroup lands on one of the four faster XCDs of the
                              * part (odd block index) are 1 + xcd_skew, the others 1 - xcd_skew times their nominal length (equal
                              * shares finish 4-6 % apart on an MI355X); 0 = equal, range -0.2 .. 0.2.  Echoed by gv_get_decomp but
                              * without effect while work items are dealt by ticket (the default; GV_DEAL=0 takes them by block index) */
} gv_decomp_info;
/* Wall time of the last ingest (gv_upload_bed / gv_upload_bed_file / gv_synth_bed), split into allocating the resident
 * layouts (hipMalloc of 100+ GB: the driver maps and wipes the pages; 0 when the buffers were reused) and filling them. */
int gv_ingest_info(gv_ctx* ctx, double* alloc_seconds, double* fill_seconds);
/* The same and more.  alloc_seconds = wall time until the resident layout was allocated AND the source prepared (the allocation
 * runs on a helper thread beside the pinned staging buffers, the chunk buffer and, for gv_upload_bed_file, the first two chunks
 * read from the file); overlap_seconds = how much of the allocation that preparation hid (wall = max, not sum). */
typedef struct {
    double alloc_seconds, fill_seconds, overlap_seconds;
    double resident_bytes;       /* genotype bytes resident after the ingest (one or two re-encoded layouts, raw rows if asked for) */
    int layout;                  /* gv_get_layout */
    int64_t expected_passes;     /* what gv_set_expected_passes said (0 = unknown) */
} gv_ingest_stats;
int gv_ingest_info2(gv_ctx* ctx, gv_ingest_stats* out);
/* Hint for gv_set_layout(.., 3) (auto), to be given before the ingest: how many ATx passes over the shard the caller expects to
 * make (a VAMP run: iterations x CG steps; 0 = unknown).  The second stripe set of layout 1 costs its bytes once more at ingest
 * (0.5-4.3 s per 100 GB, depending on whether the driver is still wiping freed memory) and makes every ATx pass ~3 % faster: it
 * pays for itself after 500-9 000 passes, whatever the shard size.  Auto builds the two sets only with a hint >= 1 000 (and room in
 * HBM); below that, and with no hint at all (ABI 3: a run that says nothing about its length is not assumed to be long), it takes
 * the one tile layout.  The drivers pass iterations x 12, bench.py the passes it is about to make. */
int gv_set_expected_passes(gv_ctx* ctx, int64_t passes);
int gv_get_decomp(gv_ctx* ctx, gv_decomp_info* out4);
/* Pins the decomposition of class cls (0 ATx, 1 two-vector ATx, 2 Ax, 3 two-vector Ax), e.g. one a deployment measured itself:
 * `tuned` is ignored, balanced_cells > 0 selects a balanced / hybrid grid (ks unused), else a uniform split of ks segments with
 * taper or geo.  Call it after the ingest; a first matvec that tunes (gv_tune_info source 1 / 2 / 4) overwrites it, one that has
 * already happened does not.  Refused when the decomposition needs more partial-sum pieces than the context holds room for, and
 * on the Ax side (cls 2, 3) when its longest K-segment is more than 4 194 303 markers (512 per marker would wrap an int32 digit
 * sum: only a shard of more markers than that can be cut so); the message names the reason.
 * Never changes a bit of output (exact integer accumulation). */
int gv_set_decomp(gv_ctx* ctx, int cls, const gv_decomp_info* in);
/* How the picks were made: *source = -1 not yet (the first matvec in kernel mode 1 makes them), 0 the cost model's first
 * candidate (tuning impossible), 1 measured on the device now (*seconds of wall time), 2 read from the cache an earlier run on
 * the same (device, N, M, kernel sources) left ($GV_TUNE_CACHE_DIR, $XDG_CACHE_HOME/gvamp_amd or ~/.cache/gvamp_amd;
 * GV_TUNE_CACHE=0 disables it), 3 fixed by an override, 4 taken from the table shipped with the library for the shapes of
 * BASELINE.json and the per-GPU shards of the headline job on an MI355X (gv_tune_builtin.h; GV_TUNE_BUILTIN=0 ignores it).
 * Picks never change results (exact integer accumulation). */
int gv_tune_info(gv_ctx* ctx, double* seconds, int* source);
/* device copy bandwidth probe: copies nbytes device->device `reps` times, returns GB/s (read+write bytes) */
int gv_copy_bandwidth(gv_ctx* ctx, size_t nbytes, int reps, double* gbps);
/* read-only stream probe with the access shape of the matvec kernels (every wave walks a contiguous run of 4 KiB blocks,
 * non-temporal 16-byte loads, nothing else): GB/s over the resident marker-major stripes when there are any, else over a
 * scratch buffer of nbytes.  The ceiling a streaming kernel can be held against on this part. */
int gv_read_bandwidth(gv_ctx* ctx, size_t nbytes, int reps, double* gbps);

/* LD-block preconditioner of every M-space CG solve (gv_cg_solve, gv_cg_solve2 / 2x / 2w).  New entry points
 * only: GV_ABI_VERSION stays 4.  kind 0 = the reference's scalar diag = tau (N-1)/N + gam2 (the default, nothing changes); kind 1 =
 * "ld": windows of `window` (32, 64 or 128) markers on global marker indices in two grids, [kW, kW+W) and [kW-W/2, kW+W/2) for k >= 0
 * (grid 1's window 0 is [0, W/2): every marker lies in one window of each grid), clipped to the shard; z = 1/2 sum over both grids of blockdiag((tau G + gam2 I)^-1) r with G the window's exact diagonal block of A^T A.  The
 * Grams come from the resident re-encoded layout (a context with raw rows only is refused, so are dense (meth) data); they are built
 * at the first solve (or gv_precond_window_gram) and dropped on a new ingest, gv_set_mask and gv_marker_stats; kind 0 releases them.  A window whose pivot is <= 1e-12 x its largest
 * diagonal, or not finite, takes the scalar rule on its markers.  With kind 1 the M-space solves run the host-driven loop, and the
 * N-space solvers gv_cg_solve_aat* are refused.  The Grams are exact int32 sums over all individuals (at most 4 per individual), so
 * kind 1 is refused above N = 2^29 - 1 where they are built, with the message of gv_ld_scores / gv_ld_band under its own name. */
int gv_set_cg_precond(gv_ctx* ctx, int kind, int window);
typedef struct gv_precond_stats {
    int kind, window;
    int64_t windows[2];          /* windows of grid 0 / 1 that overlap this shard ... */
    int64_t first_window[2];     /* ... and the global index k of the first of them */
    double resident_bytes;       /* Grams + inverses on the device */
    double build_seconds;        /* wall time of the last Gram build */
    int64_t factorisations;      /* (tau, gam2) pairs factorised so far */
    int64_t fallback_windows;    /* windows of the last factorisation on the scalar rule */
    double last_tau, last_gam2;
} gv_precond_stats;
int gv_precond_info(gv_ctx* ctx, gv_precond_stats* info);
/* W x W doubles, row-major: window k of grid (0 / 1) clipped to the shard, rows and columns past its clipped length are 0 */
int gv_precond_window_gram(gv_ctx* ctx, int grid, int64_t k, double* out);
/* z = M^-1 r for (tau, gam2) (factorises when they differ from the last factorisation) */
int gv_precond_apply(gv_ctx* ctx, double tau, double gam2, const gv_vec* r, gv_vec* z);

/* ---- LD scores and banded LD correlations of the resident genotypes (additions only: GV_ABI_VERSION stays 4) ---
 * Data: bed data with a re-encoded layout resident (the tile layout or two stripe sets), marker statistics computed; the phenotype
 * mask applies as everywhere else.  With A_nj = (a_nj - mave_j) msig_j b_nj na_n / sqrt(N), the operator of gv_ax / gv_atx,
 *   C_jk = sum_n A_nj A_nk = msig_j msig_k / N * (VV_jk - mave_k VP_jk - mave_j VP_kj + mave_j mave_k PP_jk)
 * from the exact integer sums VV = V^T V, VP = V^T P, PP = P^T P of the planes P = b na, V = a P, in that fixed fp64 order, evaluated
 * once per unordered pair (j < k) and mirrored: r_jk and r_kj are the same bits.  A marker is monomorphic if C_jj == 0 (constant among
 * the phenotyped individuals, or missing everywhere).
 *   r_jk = C_jk / sqrt(C_jj C_kk);  r_jj = 1 exactly for a polymorphic marker;  r_jk = 0 if either marker is monomorphic
 * (missing genotypes count as the mean, as the operator treats them).
 * Band: `window` = B >= 1 markers on each side in global marker order, clipped to this shard [S, S+M): the band STOPS at the shard's
 * edges (as the preconditioner's windows do), so a sharded job misses the neighbours across them.  chrom (M ints, as gv_assoc_loco
 * takes them; NULL = one chromosome): pairs on different chromosomes are outside the band.
 *   l_j = 1 + sum over k != j in the band, k polymorphic, of f(r_jk^2);  f(x) = x (adjusted == 0) or x - (1 - x) / (n - 2) with
 *   n = nonas (adjusted == 1, the LDSC estimator; needs nonas >= 3);  l_j = NaN for a monomorphic j
 *   npairs_j = the number of terms, self included (0 for a monomorphic j)
 * Row sums run in ascending k through per-block partials added in a fixed order, no atomics: two calls, both layouts and every kernel
 * mode give the same bits.  One individual adds at most 4 to an int32 sum, so N <= 2^29 - 1 needs no segmenting; a larger N is refused.
 * 1 <= window <= 8192.  Scratch is allocated for the call and released after it.  Refused with a message: methylation data, compact
 * dosage data, a context with raw rows only, statistics not computed, arguments out of range. */
int gv_ld_scores(gv_ctx* ctx, int64_t window, const int* chrom, int adjusted, double* l2 /* M */, double* npairs /* M or NULL */);
/* r: nj x (2 * window + 1) doubles, row-major, for the local markers [j0, j0 + nj): column window + d is r[j][j + d], 0 outside the band */
int gv_ld_band(gv_ctx* ctx, int64_t window, const int* chrom, int64_t j0, int64_t nj, double* r);
typedef struct gv_ld_stats {
    double seconds;              /* wall time of the last gv_ld_scores / gv_ld_band call */
    int64_t block_pairs;         /* pairs of 64-marker row groups it computed */
    double useful_macs;          /* 4 products x N x the (j, k) entries of the band it delivered, self included */
    double scratch_bytes;        /* device scratch it allocated and released */
} gv_ld_stats;
int gv_ld_info(gv_ctx* ctx, gv_ld_stats* info);
/* ---- LD scores over a window of positions, per annotation category (additions only: GV_ABI_VERSION stays 4) ----
 * The data, the planes, C_jk, r_jk, the monomorphic rule, f, and adjusted with n = nonas >= 3 are exactly those of gv_ld_scores.
 * Band: k is in the band of j iff chrom_j == chrom_k (chrom NULL: one chromosome) and |pos_k - pos_j| <= radius; the comparison is the
 * fp64 expression pos_k - pos_j <= radius for j <= k, so equal positions are always in each other's band.  pos (M doubles: bp, cM, any
 * unit radius is given in) must be finite and non-decreasing inside each maximal run of equal chrom, and each chromosome id must form a
 * single contiguous run: the band of j is then an index interval [lo_j, hi_j] with lo and hi non-decreasing and k <= hi_j <=> j >= lo_k,
 * which lets each unordered pair be evaluated once and mirrored.  The band is clipped to the shard, as above.  Reach limit:
 * hi_j - j <= 8192 for every j, the reach of gv_ld_scores' largest window.
 *   l(j, c) = a_jc + sum over k != j in the band, k polymorphic, of f(r_jk^2) * a_kc        (annot: M x ncat row-major, 1 <= ncat <= 512)
 * With annot == NULL ncat is ignored, there is one category and a = 1.  l(j, .) = NaN and npairs_j = 0 for a monomorphic j; npairs_j
 * counts the terms, self included, whatever the annotation values are (zeros and negative values are legal).
 * Summation order: per (j, c) the terms are added in ascending k, through per-block partials added in ascending block order; each term
 * is formed as the plain product f * a and then added (no fused multiply-add); the self term a_jc is added last.  No atomics: two
 * calls, both layouts and kernel modes 1 and 2 give the same bits, and so does any number of passes (below).  With pos[j] = S + j,
 * radius = B and annot == NULL the output is bit-identical to gv_ld_scores(ctx, B, chrom, adjusted, ...) (a chromosome layout with
 * non-contiguous ids is refused here, although that call serves it); an annotation of one all-ones column gives the bits of annot == NULL.
 * The per-block partial sums take (2 dmax + 1) * 64 * row groups * (8 ncat + 4) bytes, dmax the most 64-marker row groups a row group
 * reaches ahead; above a budget (2 GiB; GV_LD_PART_MB, read by gv_create) the call runs in passes over consecutive row groups, each
 * within the budget.  gv_ld_info after the call: block_pairs counts the blocks actually computed (a block that no marker reaches is
 * skipped), useful_macs = 4 N sum_j (hi_j - lo_j + 1); gv_ld_last_passes: the passes of the last LD call (1 for gv_ld_scores / band).
 * Refused with a message that names the reason: everything gv_ld_scores refuses; compact dosage data of either width, also under
 * gv_set_ld_dosage(ctx, 1) (this entry point is bed-only for now); pos == NULL; a non-finite or decreasing position and a chromosome id
 * that reappears after its run has ended (naming the first offending local marker); radius negative or not finite; a reach above 8192
 * (naming the marker and its reach); ncat outside [1, 512] when annot is given; a budget that cannot hold one row group's slots. */
int gv_ld_scores_pos(gv_ctx* ctx, const double* pos /* M */, double radius, const int* chrom /* M or NULL */, int adjusted,
                     const double* annot /* M x ncat row-major, or NULL */, int ncat,
                     double* l2 /* M x max(ncat, 1) row-major */, double* npairs /* M or NULL */);
int gv_ld_last_passes(const gv_ctx* ctx, int* passes);
/* ---- LD clumping of association results (additions only: GV_ABI_VERSION stays 4) --------------------------------
 * The data, the planes, C_jk, r_jk and the monomorphic rule are exactly those of gv_ld_scores_pos (a missing genotype counts as the
 * mean); so are the band (k is in the band of j iff same chromosome and pos_k - pos_j <= radius for j <= k), the conditions on pos and
 * chrom and the reach limit of 8192.
 * p: M host doubles (the p-values of the markers); p1 <= p2, finite and >= 0; r2 in [0, 1].
 *   E2 = { j : p_j <= p2 } may be a member of a clump, E1 = { j : p_j <= p1 } may be its index marker; a NaN p_j is in neither set.
 *   adj(j, k) iff j != k, k is in the band of j, both markers are polymorphic, both are in E2, and r_jk * r_jk >= r2 -- the product and
 *   the comparison in fp64 on the very bits gv_ld_band returns for the pair; r_jk and r_kj are the same bits, so adj is symmetric.
 *   Order: ascending p, equal p by ascending marker index.
 * Result, the sequential definition: walk E1 in that order; a marker not yet assigned becomes an index marker, index_of[j] = j, and claims
 * every still unassigned k of E2 with adj(j, k), index_of[k] = j.  Everything else -- the markers outside E2 and those of E2 \ E1 that no
 * index marker reaches -- gets index_of = -1.  A monomorphic marker of E1 is a clump of one.  n_index (may be NULL) is the number of index
 * markers.  Indices are local to the shard and the band stops at the shard's edges, as everywhere above.  The result is a function of the
 * inputs alone: two calls, both layouts and kernel modes 1 and 2 give the same values.
 * The adjacency is held as bit words, 8 * 64 * (2 dmax + 1) * row groups bytes (dmax as above), allocated for the call and released
 * after it; only the blocks that hold an in-band pair AND a marker of E2 in both row groups are computed.  gv_ld_info after the call:
 * seconds, block_pairs = the blocks computed, useful_macs = 4 N x the ordered in-band pairs (j, k) with both in E2, self included, and
 * the scratch bytes.  gv_ld_clump_last: the rounds the selection of the index markers took (0 with E1 empty; it may depend on the
 * scheduling of the device, the result does not), |E1| and |E2|; gv_ld_clump_seconds: the block pass and the selection apart.
 * Refused with a message that names the reason: everything gv_ld_scores_pos refuses (dosage codes with or without gv_set_ld_dosage,
 * methylation data, raw rows only, statistics not computed, pos == NULL, a non-finite or decreasing position, a chromosome id that
 * reappears, a reach above 8192, a non-finite or negative radius); p or index_of NULL; p1, p2 or r2 not finite; p1 > p2; p1 < 0; r2
 * outside [0, 1].  M == 0 returns 0 and touches nothing. */
int gv_ld_clump(gv_ctx* ctx, const double* pos /* M */, double radius, const int* chrom /* M or NULL */,
                const double* p /* M */, double p1, double p2, double r2,
                int64_t* index_of /* M */, int64_t* n_index /* 1, or NULL */);
int gv_ld_clump_last(const gv_ctx* ctx, int* rounds, int64_t* n_e1, int64_t* n_e2);   /* of the last gv_ld_clump */
int gv_ld_clump_seconds(const gv_ctx* ctx, double* block_pass, double* selection);    /* of the last gv_ld_clump */
/* ---- LD of 8-bit dosage codes (additions only: GV_ABI_VERSION stays 4) ----------------------------------------
 * gv_set_ld_dosage(ctx, 1): gv_ld_scores, gv_ld_band and gv_ld_info accept a context whose resident data are 8-bit dosage codes and
 * whose mask is set.  Per context, default 0, it outlives the dataset; with 0 nothing changes by a bit or by a message.  Marker
 * statistics are not needed (mave and msig do not enter).  Still refused, each by its own message: 16-bit codes ("16-bit codes"),
 * methylation data, no mask, and the window / adjusted / band-row checks above.
 * Definition, in exact integers up to one rounding per quantity.  b_jn = 0 at the reserved code 255 when the codes were uploaded under
 * gv_set_dosage_missing, 1 otherwise (with the option off 255 is the value 255); P_jn = b_jn na_n, V_jn = (code_jn - 128) P_jn;
 *   VV_jk = sum V_j V_k, VP_jk = sum V_j P_k, PP_jk = sum P_j P_k, c_j = sum P_j, T_j = sum V_j            (sums over the individuals)
 *   X_jk = c_j c_k VV_jk - c_j T_k VP_jk - c_k T_j VP_kj + T_j T_k PP_jk     = c_j c_k sum_n (code_j - mu'_j)(code_k - mu'_k) P_j P_k
 * formed in 128-bit integers and converted to fp64 correctly rounded (a missing entry counts as the mean);
 *   r_jk = fl(X_jk) / sqrt(fl(X_jj) fl(X_kk)) for j < k, mirrored;  monomorphic iff X_jj == 0 (exact for a constant and for an
 *   all-missing row);  r_jj = 1 for a polymorphic marker, r_jk = 0 if either marker is monomorphic.
 * Band, chromosomes, l_j, npairs_j, the adjusted estimator with n = nonas, NaN and 0 for a monomorphic j: as above.  The sums are int32
 * MFMA sums over at most 131 071 individuals (GV_DOSAGE_MFMA_SEG lowers it) added in int64: no bit depends on the segment length, the
 * kernel instantiation or the call.  gv_ld_stats.useful_macs counts 1 product where every marker shares the presence pattern na (no
 * reserved code in the shard), 4 otherwise (or under GV_DOSAGE_NA_KERNELS=1).  N <= 2^29 - 1. */
int gv_set_ld_dosage(gv_ctx* ctx, int on);
int gv_get_ld_dosage(const gv_ctx* ctx, int* on);
/* ---- LD-block preconditioner of 8-bit dosage codes (additions only: GV_ABI_VERSION stays 4) ------------------
 * While gv_set_ld_dosage(ctx, 1) is in force and 8-bit codes are resident, gv_set_cg_precond(ctx, 1, window) is accepted, and
 * gv_precond_info, gv_precond_window_gram, gv_precond_apply and every M-space solve work as on bed data.  With the option off (the
 * default) every call and every message is what it was.  Windows, the two grids, clipping to the shard, B = tau G + gam2 I, the
 * pivot rule and the apply are those of gv_set_cg_precond above; only the Gram differs.
 * Definition.  A_nj = (code_nj - mu'_j) s_j b_nj na_n / sqrt(N) with s_j = msig_j * scale is the matrix gv_ax / gv_atx apply to
 * compact data.  G is the window's exact diagonal block of A^T A,
 *   G_jk = s_j s_k / N * X_jk / (c_j c_k)
 * with the integers X_jk, c_j, T_j of gv_set_ld_dosage above: X formed in 128 bits, converted to fp64 correctly rounded.  The ONE
 * fp64 evaluation order, symmetric in j and k:
 *   G_jk = ((s_j * s_k) * (1 / N)) * (fl(X_jk) / (fl(c_j) * fl(c_k))),    s_j = msig_j * scale,  1 / N one division
 * so G_jk and G_kj are the same bits (every product is commutative and X_jk = X_kj exactly) and the mirror image of a block is a
 * copy.  A row with c_j = 0 (no present individual) contributes exact zeros; a constant row has X_jj = 0, hence G_jj = 0, exactly.
 * Needs the mask and the marker statistics (msig enters).  The Grams are built at the first solve or gv_precond_window_gram and
 * dropped where the bed Grams are and also by a new dosage upload or synthesis, gv_set_dosage_missing and gv_set_ld_dosage.  The sums
 * are int32 MFMA sums over at most 131 071 individuals added in int64: the Grams are the same bits for every segment length, for the
 * one-product and the four-product kernel on data without a reserved code, and across calls.
 * Still refused, each by a message that names its reason: 16-bit codes ("16-bit codes"), methylation data, the N-space solvers and
 * gv_cg_warm::ata_v_b under kind 1, N > 2^29 - 1.  If kind 1 was accepted and the option is then switched off, the next solve,
 * gv_precond_apply or gv_precond_window_gram refuses with a message that names gv_set_ld_dosage. */
/* ---- many weight vectors in one pass: Z = A W (additions only: GV_ABI_VERSION stays 4) ---------------------
 * gv_score_dev: out[j] = data::Ax(x[j]) for j = 0 .. C-1.  Column j is bit-identical to gv_ax_dev(ctx, x[j], out[j]) called alone on
 * the same context: in every kernel mode, on every resident layout, for every data kind gv_ax_dev serves, with or without a
 * communicator, whatever C is, whatever position the column has and whatever the other columns hold (a column with a NaN or an
 * infinity is NaN as gv_ax_dev makes it; its neighbours are untouched).
 * Path.  In kernel mode 1 on the tile layout (gv_get_layout() == 2), 2-bit genotypes, one rank, and C >= gv_score_stats.min_cols, a
 * kernel of its own multiplies up to cols_per_pass columns per pass over the genotypes (GV_SCORE_PATH_KERNEL).  Everywhere else --
 * two stripe sets, kernel modes 0 and 2, methylation and dosage data, a communicator or gv_debug_force_multi, an empty shard, fewer
 * columns -- the dispatcher behind gv_ax_dev / gv_ax2_dev runs, in pairs where a two-vector pass exists and singly otherwise
 * (GV_SCORE_PATH_FALLBACK).  GV_SCORE_KERNEL=1 / 0 (development, read by gv_create per context) makes min_cols 1 / unreachable.
 * Edge rules.  C == 0 succeeds and does nothing.  Refused with a message: C < 0; NULL arrays or handles; an x that is not M-space or
 * an out that is not N-space; two outputs that are the same vector; an output that is also an input; marker statistics or mask missing
 * (the message of gv_ax_dev).  Inputs may repeat.
 * The call leaves the context as it found it: the tuned decompositions, the ticket counter, the digit and operand buffers of the other
 * products and the CG work vectors are not touched by the kernel path; a gv_ax_dev, gv_ax2_dev or gv_lmmse_mult after it returns the
 * bits it returned before.  It is enqueued on the context's stream like gv_ax_dev.
 * Scratch (kernel path): digits, int32 partial sums and scalars of one pass, gv_score_stats.scratch_bytes in all.  It is OWNED BY THE
 * CONTEXT: allocated or grown by the call that needs it, kept for the next call, freed with the dataset (gv_set_dims) and by
 * gv_destroy.  A call that cannot get it fails with the byte count in the message.
 * No K-segment of a pass spans more than 4 194 303 markers (the int32 digit sums); a shard that no split into 64 segments serves is
 * refused.  GV_SCORE_COLS=<4|8|16> pins the columns per pass and GV_SCORE_KS=<k> the K-segments (development, read by gv_create per
 * context; gv_create refuses other values, the call refuses a k that breaks the bound); neither changes a bit.
 * gv_score: the same on host arrays: column j of W at W + j * M, column j of the result at out + j * 4 * mbytes; returns when out is
 * filled.  gv_score_info: the last gv_score_dev / gv_score call of the context.
 * A context joined to others (gv_comm_init*, a marker-sharded job): x[j] holds this rank's M entries of column j, out[j] is the sum
 * over the ranks, the same bits on every rank.  Every column is one collective (two for a pair): EVERY rank of the job makes the call,
 * with the same C, at the same place in its sequence of collective calls, under the same mask and kernel mode -- a rank without
 * markers (M == 0) included, which adds zeros.  A rank that stays away leaves its peers waiting.  The sum over the ranks is another
 * rounding than the sum of one context over all markers: a sharded result equals a one-rank result to the accuracy of gv_ax_dev, not
 * by bits (tests/test_gpu_sharded_products.py). */
#define GV_SCORE_PATH_KERNEL 1
#define GV_SCORE_PATH_FALLBACK 2
#define GV_SCORE_COLS_DEFAULT 8
typedef struct gv_score_stats {
    int path;                    /* 0 no call yet, GV_SCORE_PATH_KERNEL, GV_SCORE_PATH_FALLBACK */
    int cols_per_pass;           /* kernel: 4, 8 or 16 (the last pass may run narrower); fallback: 2 where a two-vector pass exists, else 1 */
    int ksegs;                   /* kernel: K-segments of a pass; fallback: 0 */
    int min_cols;                /* the fewest columns for which the kernel is the path where it applies */
    int64_t columns;             /* C */
    int64_t passes;              /* passes over the genotypes */
    uint64_t scratch_bytes;      /* kernel: bytes of scratch the call needed; fallback: 0 */
    double seconds;              /* host wall time of the call (gv_score_dev enqueues: its device work may still be running) */
} gv_score_stats;
int gv_score_dev(gv_ctx* ctx, int64_t C, const gv_vec* const* x /* C handles, GV_SPACE_M */, gv_vec* const* out /* C handles, GV_SPACE_N */);
int gv_score(gv_ctx* ctx, int64_t C, const double* W /* column j at W + j*M */, double* out /* column j at out + j*4*mbytes */);
int gv_score_info(const gv_ctx* ctx, gv_score_stats* out);

/* ---- many phenotype vectors in one pass: R = A^T Y, and a marginal screen on it (additions only: GV_ABI_VERSION stays 4; DESIGN.md
 * section 23) ------------------------------------------------------------------------------------------------------------------------
 * gv_atxm_dev: out[j] = data::ATx(p[j]) for j = 0 .. C-1.  Column j is bit-identical to gv_atx_dev(ctx, p[j], out[j]) called alone on
 * the same context: in every kernel mode, on every resident layout, for every data kind gv_atx_dev serves, with or without a
 * communicator, whatever C is, whatever position the column has and whatever the other columns hold (a column with a NaN or an
 * infinity comes out as gv_atx_dev makes it; its neighbours do not move).  As in gv_atx_dev, p is used as given: the caller zeroes NA
 * and pad slots.
 * Path.  In kernel mode 1 on the tile layout (gv_get_layout() == 2), 2-bit genotypes, M > 0 and C >= gv_atxm_stats.min_cols, a kernel
 * of its own multiplies up to cols_per_pass columns per pass over the genotypes (GV_ATXM_PATH_KERNEL).  ATx issues no collective, so a
 * communicator or gv_debug_force_multi does not change the path.  Everywhere else -- two stripe sets, kernel modes 0 and 2, methylation
 * and dosage data, an empty shard, fewer columns -- the dispatcher behind gv_atx_dev / gv_atx2_dev runs, in pairs where a two-vector
 * pass exists and singly otherwise (GV_ATXM_PATH_FALLBACK).  min_cols is 4, measured.  GV_ATXM_KERNEL=1 / 0
 * (development, read by gv_create per context) makes min_cols 1 / unreachable.
 * 8-bit dosage codes while the fixed-point route is in force (gv_get_dosage_route reports in_force == 1: requested, 8-bit codes, the
 * plain kernels) with M > 0 have a kernel of their own: GV_ATXM_PATH_KERNEL with cols_per_pass 4 or 8
 * (GV_ATXM_COLS pins it; the default is GV_ATXM_DENSE_COLS_DEFAULT), ksegs the int32 segments of the one-vector product, and a min_cols
 * of its own, 3, which GV_ATXM_KERNEL sets the same way.  The contract is the one above: every sum of that route is an exact integer,
 * a column is quantised and rounded by the functions gv_atx_dev runs, and it is bit-identical to gv_atx_dev of that column alone.  Its
 * scratch is the context's (the formula: gv_dense_atxm_plan.h); the digit and partial-sum buffers of gv_atx_dev / gv_ax_dev on that route
 * are not touched.  Route 0, 16-bit codes, a shard with reserved codes under gv_set_dosage_missing, GV_DOSAGE_NA_KERNELS=1 and
 * methylation data keep the fallback.
 * Edge rules.  C == 0 succeeds and does nothing.  Refused with a message: C < 0; NULL arrays or handles; a p that is not N-space or an
 * out that is not M-space; two outputs that are the same vector; an output that is also an input; marker statistics missing (the
 * message of gv_atx_dev).  Inputs may repeat.
 * The call leaves the context as it found it: the tuned decompositions, the ticket counter (work items are dealt by block index), the
 * digit, scalar and partial-sum buffers of the other products, the reduction partials and the CG work vectors are not touched by the
 * kernel path.  It is enqueued on the context's stream like gv_atx_dev, and counted in the ATx counters (C products, its passes).
 * Scratch (kernel path): digits, int32 partial sums and scalars of one pass, gv_atxm_stats.scratch_bytes in all (the formula:
 * gv_atxm_plan.h).  It is OWNED BY THE CONTEXT: allocated or grown by the call that needs it, kept for the next call, freed with the
 * dataset (gv_set_dims) and by gv_destroy.  A call that cannot get it fails with the byte count in the message.
 * GV_ATXM_COLS=<4|8> pins the columns per pass and GV_ATXM_KS=<k> the K-segments (development, read by gv_create per context;
 * gv_create refuses other values; k is clipped to the K-steps there are); neither changes a bit.
 * gv_atxm: the same on host arrays: column j of Y at Y + j * 4 * mbytes, column j of the result at out + j * M; the staged copy of a
 * column is masked as gv_atx masks its own; returns when out is filled.  gv_atxm_info: the last gv_atxm_dev / gv_atxm / gv_screen_dev.
 *
 * gv_screen_dev: the marginal association screen of C prepared phenotype columns u[c] (N-space) against every marker.  u[c] is zero
 * at NA and pad slots, centred over the n = nonas phenotyped individuals of the context's mask and scaled by
 * sqrt((n - 1) / sum (y - mean)^2).  With z = gv_atxm_dev(u), per marker and column, in this order of fp64 roundings:
 *     a  = fl(fl(sqrt(N)) / (n - 1))          (host, once)
 *     r  = fl(z a)                            the Pearson correlation of the mean-imputed genotype column with the phenotype
 *     om = fma(-r, r, 1)                      1 - r^2 in one rounding
 *     t  = fl(r fl(sqrt(fl((n - 2) / om))))   p = gvp::t_two_sided(|t|, n - 2)
 * om <= 0 gives t = +-inf (the sign of r) and p = 0.  A marker without variance among the phenotyped present genotypes (monomorphic
 * or all missing: sumsqx == 0 in the expression of the association test) gives NaN in all three outputs.  (The other half of that
 * test's rule, fewer than three present genotypes, does not apply: under mean imputation the degrees of freedom are n - 2 for every
 * marker.)  r, t, p are M-space; t and p may be NULL arrays.  All outputs are distinct vectors, none is an input.
 * Refused with a message: everything gv_atxm_dev refuses; n < 3; methylation and dosage data; marker statistics of alpha_scale != 1.
 * A context joined to others (a marker-sharded job): gv_atxm_dev and gv_screen_dev issue no collective and every output is a quantity
 * of one marker, so a rank may call them alone and the outputs of the ranks, put side by side in marker order, are the output of one
 * context on all markers bit for bit -- PROVIDED every rank has set the same mask (gv_set_mask with the same bytes and nonas: the
 * statistics of a marker and n depend on it) and passes the same columns.  On a rank without markers the calls succeed and write
 * nothing.
 *
 * Screens on dosage data (additions only).  gv_set_screen_dosage(ctx, 1): gv_screen_dev, gv_screen_cov_set and
 * gv_screen_cov_dev accept a context whose resident data are dosage codes -- 8 or 16 bits, with or without missing entries
 * (gv_set_dosage_missing), on either route.  The default is 0: every call and message is what it was.  The setting outlives the dataset
 * and is read by every call; nothing is derived from it, so nothing goes stale.  Methylation data stay refused either way.
 * Definition.  With b the code, na = 1 at a present entry (0 at a reserved code), mu' the mean code over the phenotyped present entries
 * and q = sum_n ((b - mu') na)^2 over the phenotyped individuals, the marker statistics give msig^2 scale^2 q = n - 1 (alpha_scale = 1):
 * the column (b - mu') msig scale na has squared norm n - 1, the identity the bed screens rest on.  So the formulas above and those of
 * gv_screen_cov_dev hold unchanged, with the same order of roundings: r = fl(z a) is the Pearson correlation of the mean-imputed dosage
 * (a missing entry counts as the marker's mean) with the phenotype, nu = n - 2 (n - 2 - K adjusted), and in the adjusted screen
 * sxx_j = fl(fl(scale scale) q_j) takes the place of fl((n - 1) / msig^2): beta and se are per unit of the value scale * code, per allele
 * copy at the default scales.  A marker with q == 0 -- constant over the phenotyped present entries, or all missing; exact in code units
 * whatever the scale -- gives NaN in every output.  q is the sum the statistics pass forms for msig, kept per marker beside mu'
 * (the decision is taken from q itself, never from msig == 1); it goes stale and is restored with the marker statistics.
 * The products run on whatever path gv_atxm_dev takes for the context, so column independence on the bits holds as above.
 * Refused as on bed data, by the same messages: alpha_scale != 1, n < 3 or nu < 1, every vector and handle check. */
int gv_set_screen_dosage(gv_ctx* ctx, int on);
int gv_get_screen_dosage(const gv_ctx* ctx, int* on);
#define GV_ATXM_DENSE_COLS_DEFAULT 8
#define GV_ATXM_PATH_KERNEL 1
#define GV_ATXM_PATH_FALLBACK 2
#define GV_ATXM_COLS_DEFAULT 8
typedef struct gv_atxm_stats {
    int path;                    /* 0 no call yet, GV_ATXM_PATH_KERNEL, GV_ATXM_PATH_FALLBACK */
    int cols_per_pass;           /* kernel: 4 or 8 (the last pass may run narrower); fallback: 2 where a two-vector pass exists, else 1 */
    int ksegs;                   /* kernel: K-segments of a pass; fallback: 0 */
    int min_cols;                /* the fewest columns for which the kernel is the path where it applies */
    int64_t columns;             /* C */
    int64_t passes;              /* passes over the genotypes */
    uint64_t scratch_bytes;      /* kernel: bytes of scratch the call needed; fallback: 0 */
    double seconds;              /* host wall time of the call (gv_atxm_dev enqueues: its device work may still be running) */
} gv_atxm_stats;
int gv_atxm_dev(gv_ctx* ctx, int64_t C, const gv_vec* const* p /* C handles, GV_SPACE_N */, gv_vec* const* out /* C handles, GV_SPACE_M */);
int gv_atxm(gv_ctx* ctx, int64_t C, const double* Y /* column j at Y + j*4*mbytes */, double* out /* column j at out + j*M */);
int gv_atxm_info(const gv_ctx* ctx, gv_atxm_stats* out);
int gv_screen_dev(gv_ctx* ctx, int64_t C, const gv_vec* const* u /* C, GV_SPACE_N */, gv_vec* const* r, gv_vec* const* t,
                  gv_vec* const* p /* C each, GV_SPACE_M; t and p may be NULL arrays */);

/* ---- principal components of the resident genotypes by block subspace iteration (additions only: GV_ABI_VERSION stays 4; DESIGN.md
 * section 24) ------------------------------------------------------------------------------------------------------------------------
 * A is the matrix gv_ax_dev / gv_atx_dev apply (mean-imputed, centred, scaled by msig, divided by sqrt(N), rows of NA and pad
 * individuals zero) and G = (N / Mt) A A^T the genetic relationship matrix over the markers of all ranks.  gv_pca_dev returns the k
 * largest eigenpairs (eval[i], u[i]) of G, eval descending; u[i] is N-space, of unit 2-norm, zero at NA and pad slots, and its entry of
 * largest magnitude is positive (the lowest index on ties).
 * Algorithm, on a block of L vectors, k <= L <= GV_PCA_MAX_BLOCK, the caller giving the starting block q0 (not modified):
 *     Q <- orth(mask q0)
 *     each iteration:  B = gv_atxm_dev(Q);  Y = fl((N / Mt) gv_score_dev(B));  T = sym(Q^T Y) = V Theta V^T, Theta descending;
 *                      U = Q V;  R = Y V - U Theta;  r_i = ||R_i||_2
 *     stop when r_i <= tol * theta_i for every i < k; otherwise Q <- orth(Y), up to max_iter iterations.
 * orth is CholeskyQR applied twice (S = Y^T Y, S = R^T R, Y <- Y R^-1).  A pivot d of the factorisation that is not above
 * 32 * 2^-52 times its own diagonal entry of S counts as not positive: the block is rank deficient to working precision.
 * Everything between two products runs in kernels of gv_pca.hip, in fp64, in an order of operations that is a function of (npad, L)
 * alone: no atomics, fixed grids, a fixed rotation order in the eigensolver.  The products are bit-identical per column whatever their
 * path and pins (GV_SCORE_COLS / GV_SCORE_KS / GV_SCORE_KERNEL, GV_ATXM_COLS / GV_ATXM_KS / GV_ATXM_KERNEL, a communicator), so u, eval
 * and resid are bit-reproducible across them.  Per iteration the host reads back theta[0..k), r[0..k) and the Cholesky flag through the
 * scalar mailbox, once; that read-back is the convergence decision.  Everything but B is N-space, identical on every rank behind Ax's
 * own all-reduce: a sharded job needs no collective of its own.
 * Running out of max_iter is not an error: the call returns 0 with gv_pca_stats.converged = 0 and the last Ritz pairs and residuals.
 * resid[i] is the residual of (eval[i], u[i]) as the iteration formed it from the Y it already had: ||G u_i - eval_i u_i|| up to the
 * products' own error.
 * Refused with a message, no output written: k < 1; L < k; L > GV_PCA_MAX_BLOCK; L > min(nonas, Mt); tol not a positive finite number;
 * max_iter < 1; NULL arrays or handles; vectors that are not N-space, of another context or of earlier dimensions; two outputs that
 * are the same vector; an output that is also an input; mask or marker statistics missing (the message of gv_ax_dev); a Cholesky
 * pivot that is not positive by the rule above (a rank-deficient starting block, or rank(G) < L; the message names the threshold).
 * Served wherever gv_score_dev / gv_atxm_dev are: every data kind, layout and kernel mode, with or without a communicator.
 * Scratch: four N-space panels and one M-space panel of L columns and a few small buffers, gv_pca_stats.scratch_bytes in all, OWNED BY
 * THE CONTEXT: grown by the call that needs it, kept for the next, freed with the dataset (gv_set_dims) and by gv_destroy.  The call
 * leaves the context as it found it, by the rule of gv_score_dev / gv_atxm_dev; it writes the reduction scalars as gv_vec_dots does.
 * gv_pca_loadings_dev: v[i] = fl(c_i * gv_atx_dev(u[i])), c_i = fl(fl(sqrt(fl(N / Mt))) / fl(sqrt(eval[i]))): the right singular
 * vectors in M-space (this rank's markers), one rounding after the product; k <= GV_PCA_MAX_BLOCK, eval[i] positive and finite.
 * gv_pca_info: the last successful gv_pca_dev of the context.
 * A context joined to others (a marker-sharded job): the relationship matrix is that of all Mt markers.  gv_pca_dev is a sequence of
 * collectives (L columns of gv_score_dev's fallback per iteration) and nothing else crosses the ranks: EVERY rank makes the call -- a
 * rank with fewer markers than L, or with none, included: the block is bounded by min(nonas, Mt) -- with the same k, L, tol and
 * max_iter, the same bits in q0 and the same mask.  Then the N-space state is the same bits on every rank, every rank takes the same
 * decisions (the Cholesky flag, convergence) from the same scalars and leaves the loop in the same iteration; u, eval, resid and
 * gv_pca_info's iterations / converged are identical on every rank.  A rank whose q0, mask or arguments differ decides differently
 * and leaves its peers waiting in a collective: the caller's to guarantee, nothing checks it.  gv_pca_loadings_dev issues no
 * collective; v holds this rank's M markers of the Mt-vector. */
#define GV_PCA_MAX_BLOCK 32
typedef struct gv_pca_stats {
    int iterations;              /* iterations run (each one pass of L columns through both batch products) */
    int converged;               /* 1: r_i <= tol * theta_i for every i < k; 0: max_iter ran out */
    int block;                   /* L */
    int pad_;
    int64_t cols_atxm;           /* columns through gv_atxm_dev's product in all */
    int64_t cols_score;          /* columns through gv_score_dev's product in all */
    uint64_t scratch_bytes;      /* bytes of the work panels and small buffers */
    double seconds_products;     /* device time in the two batch products (events on the context's stream) */
    double seconds_panel;        /* device time in the panel kernels: orthonormalisation, Rayleigh-Ritz, rotation, residuals */
    double seconds;              /* host wall time of the call */
} gv_pca_stats;
int gv_pca_dev(gv_ctx* ctx, int k, int L, const gv_vec* const* q0 /* L, GV_SPACE_N, not modified */, double tol, int max_iter,
               gv_vec* const* u /* k, GV_SPACE_N */, double* eval /* k */, double* resid /* k */);
int gv_pca_loadings_dev(gv_ctx* ctx, int k, const gv_vec* const* u, const double* eval, gv_vec* const* v /* k, GV_SPACE_M */);
int gv_pca_info(const gv_ctx* ctx, gv_pca_stats* out);

/* ---- pairwise kinship (KING-robust) of the resident genotypes (additions only: GV_ABI_VERSION stays 4) -----------
 * Data: bed data resident in the TILE LAYOUT (gv_get_layout() == 2; kernel mode 1 or 2, the layout is the same), one rank.  The
 * phenotype mask and the marker statistics are NOT consulted and need not exist: relatedness is a property of the genotypes, and a call
 * before gv_set_mask works.
 * For individual n and marker m, a in {0, 1, 2} is the allele count the re-encoding stores (r' = a; r' = 3: missing).  The planes:
 *   P = present,   H = [a = 1] P,   D = (a - 1) P   (-1, 0 or 1)
 * `use` (M bytes, one per marker of the shard, non-zero = used; NULL = every marker) multiplies all three.  Pad markers and pad
 * individuals contribute nothing.  The five integer counts of a pair (i, j), summed over the used markers:
 *   nsnp = sum P_i P_j    hethet = sum H_i H_j    het_i = sum H_i P_j    het_j = sum P_i H_j    dd = sum D_i D_j
 * and from them
 *   homhom = nsnp - het_i - het_j + hethet
 *   ibs0   = (homhom - dd) / 2          (exact: the markers where both are present and opposite homozygotes)
 *   d2     = 4 ibs0 + (het_i - hethet) + (het_j - hethet)          (= sum over both present of (a_i - a_j)^2)
 * Kinship is the between-family KING-robust estimator (Manichaikul et al. 2010):
 *   mn  = min(het_i, het_j)                       (int64)
 *   kin = 0.5 - (double)d2 / (double)(4 mn)       one correctly rounded division, one subtraction
 *   kin = NaN if mn == 0                          (a NaN never passes a cutoff)
 * The expression is symmetric in exact integers, so kin[i][j] and kin[j][i] are the same bits.  One marker adds at most 1 in magnitude
 * to any sum: no int32 sum is segmented for M <= 2^31 - 1, and a larger shard is refused.
 * gv_king_block: the dense rectangle of individuals [i0, i0 + ni) x [j0, j0 + nj), row-major.  counts: 5 int32 per entry in the order
 *   nsnp, hethet, ibs0, het_i, het_j, het_i being the row individual's and het_j the column individual's.  Either output may be NULL.
 *   The diagonal gets the same formula (0.5 wherever the individual has a heterozygote).
 * gv_king_pairs: every pair i < j < N with kin >= cutoff (-inf: every pair whose kin is a number).  *n_found is always set to the number
 *   of such pairs; the arrays are written only when *n_found <= cap, and then in ascending (i, j) order, het_i being individual i's.
 *   With *n_found > cap nothing is promised about the arrays, the return code is still 0, and the caller calls again with a larger cap.
 *   Delivered order and content are a function of the data alone: two calls give the same bytes.  N^2 outputs never exist.
 * Scratch is taken for the call and freed after it.
 * Refused with a message, no output written: dosage or methylation data; raw rows only; two stripe sets resident (upload under the tile
 * layout, gv_set_layout(ctx, .., 2)); a job of more than one rank (the counts are sums over ALL ranks' markers; the integer all-reduce
 * is not built); NULL n_found, NULL arrays with cap > 0; a rectangle outside [0, N); cap < 0; a cutoff that is NaN or +inf. */
typedef struct gv_king_stats {
    double seconds;              /* wall time of the last gv_king_block / gv_king_pairs call */
    int64_t block_pairs;         /* pairs of 64-individual groups it computed */
    int64_t used_markers;        /* markers of the shard that counted (use != 0) */
    int64_t pairs;               /* pairs delivered: ni * nj of a rectangle, the N (N - 1) / 2 pairs gv_king_pairs decided */
    double useful_macs;          /* 5 products x used_markers x pairs */
    double scratch_bytes;        /* device scratch it allocated and released */
} gv_king_stats;
int gv_king_block(gv_ctx* ctx, const uint8_t* use /* M or NULL */, int64_t i0, int64_t ni, int64_t j0, int64_t nj,
                  double* kin /* ni * nj or NULL */, int32_t* counts /* ni * nj * 5 or NULL */);
int gv_king_pairs(gv_ctx* ctx, const uint8_t* use /* M or NULL */, double cutoff, int64_t cap, int32_t* pi, int32_t* pj, double* kin,
                  int32_t* counts /* cap (x 5) each */, int64_t* n_found);
int gv_king_info(gv_ctx* ctx, gv_king_stats* info);

/* ---- standardised genetic relationship matrix (GRM) of the resident genotypes (additions only: GV_ABI_VERSION stays 4; DESIGN.md
 * section 28) ------------------------------------------------------------------------------------------------------------------------
 * Data: bed data resident in the TILE LAYOUT (gv_get_layout() == 2; kernel mode 1 or 2), one rank, as gv_king_*.  The phenotype mask and
 * the marker statistics are NOT consulted and need not exist; frequencies are taken over all N individuals of the shard.
 * For individual i and marker m, a in {0, 1, 2} is the allele count the re-encoding stores (r' = a; r' = 3: missing); `use` is one byte
 * per marker of the shard (non-zero = selected; NULL = every marker).  Per marker, in exact integers:
 *   n_m = number of individuals present        s_m = sum of a over them
 * Marker m COUNTS iff use[m] && n_m > 0 && 0 < s_m < 2 n_m (selected, somebody present, not monomorphic).  Its weights, in exactly these
 * fp64 operations, each correctly rounded:
 *   mu = (double)s / (double)n        h = mu * (1.0 - 0.5 * mu)        rs = 1.0 / sqrt(h)
 * A marker that does not count has mu = rs = 0.  The entries:
 *   z_im = ((double)a - mu) * rs      where individual i is present at a counting marker m, else 0
 * The common-marker count M_ij is the number of counting markers at which both i and j are present: an exact integer, int32.
 *   S_ij = sum_m z_im z_jm            in fp64, over the markers of the shard in ascending order of K-step (4 markers), one accumulator;
 *                                     the order is a function of (M, use) alone
 *   A_ij = S_ij / (double)M_ij        one correctly rounded division; A_ij = NaN when M_ij = 0 (a NaN never passes a cutoff)
 * This is GCTA's estimator (Yang et al. 2011): the denominator is per pair, not a global M.  A[i][j] and A[j][i] are the same bits, the
 * diagonal gets the same formula, two calls give the same bytes, and the bits of an entry do not depend on the rectangle or the list it
 * was asked through.  Pad markers and pad individuals contribute nothing.  M <= 2^31 - 1, as gv_king_*.
 * gv_grm_weights: the pre-pass alone: mu and rs of every marker of the shard (either may be NULL) and *n_used, the markers that count.
 * gv_grm_block: the dense rectangle of individuals [i0, i0 + ni) x [j0, j0 + nj), row-major.  Either output may be NULL.
 * gv_grm_pairs: every pair i < j < N with A_ij >= cutoff (-inf: every pair whose value is a number), by the protocol of gv_king_pairs:
 *   *n_found is always set; pi, pj, a and m_common are written only when *n_found <= cap, and then in ascending (i, j) order; with
 *   *n_found > cap the return code is still 0 and the caller calls again with a larger cap.  diag (A_ii) and diag_m (M_ii), N values each,
 *   are written by every successful call that passes them: a sparse GRM needs its diagonal, and N x N never exists.
 * Scratch is taken for the call and freed after it.
 * Refused with a message, no output written: dosage or methylation data; raw rows only; two stripe sets resident (upload under the tile
 * layout, gv_set_layout(ctx, .., 2)); a job of more than one rank (S and M_ij are sums over ALL ranks' markers; the all-reduce is not
 * built); NULL n_found, NULL arrays with cap > 0; a rectangle outside [0, N); cap < 0; a cutoff that is NaN or +inf. */
typedef struct gv_grm_stats {
    double seconds;              /* wall time of the last gv_grm_weights / gv_grm_block / gv_grm_pairs call */
    int64_t block_pairs;         /* pairs of 64-individual groups it computed */
    int64_t counting_markers;    /* markers of the shard that counted */
    int64_t dropped_markers;     /* selected markers that did not: monomorphic or never present */
    int64_t pairs;               /* pairs delivered: ni * nj of a rectangle, the N (N - 1) / 2 pairs gv_grm_pairs decided, 0 of the weights */
    double useful_macs;          /* counting_markers x pairs */
    double scratch_bytes;        /* device scratch it allocated and released */
    int64_t passes;              /* launches of the block kernel: 1 for a rectangle or a pair list, the tiles of gv_grm_apply (below) */
    int64_t blocks_computed;     /* blocks those launches computed; gv_grm_apply computes no block twice: always block_pairs */
} gv_grm_stats;
int gv_grm_weights(gv_ctx* ctx, const uint8_t* use /* M or NULL */, double* mu /* M or NULL */, double* rs /* M or NULL */, int64_t* n_used);
int gv_grm_block(gv_ctx* ctx, const uint8_t* use /* M or NULL */, int64_t i0, int64_t ni, int64_t j0, int64_t nj,
                 double* a /* ni * nj or NULL */, int32_t* m_common /* ni * nj or NULL */);
int gv_grm_pairs(gv_ctx* ctx, const uint8_t* use /* M or NULL */, double cutoff, int64_t cap, int32_t* pi, int32_t* pj, double* a,
                 int32_t* m_common /* cap each */, double* diag /* N or NULL */, int32_t* diag_m /* N or NULL */, int64_t* n_found);
int gv_grm_info(gv_ctx* ctx, gv_grm_stats* info);

/* ---- GRM-times-panel product and Haseman-Elston regression, the matrix never stored (additions only: GV_ABI_VERSION stays 4; DESIGN.md
 * section 30) ------------------------------------------------------------------------------------------------------------------------
 * Data, `use`, weights, S_ij, M_ij and A_ij are exactly gv_grm_block's, to the bit.  Three symmetric N x N operators, none ever stored,
 * each with a zero diagonal and zero for a pair with M_ij = 0 (a NaN never enters a sum):
 *   G0_ij = 1        G1_ij = A_ij        G2_ij = __dmul_rn(A_ij, A_ij)   (the square is rounded before anything is multiplied into it)
 * gv_grm_apply(ctx, use, C, w, g0, g1, g2), 1 <= C <= GV_GRM_APPLY_MAX_COLS, w N x C row-major on the host and finite:
 *   gp[i][c] = sum_j Gp_ij w[j][c]        (each of g0, g1, g2 N x C row-major on the host, or NULL)
 * The order of the sum is part of the contract and a function of N alone.  With S a group of 64 consecutive individuals (64 S ..):
 *   b_S      = the chain over j ascending in S, from +0.0, of acc = __dadd_rn(acc, __dmul_rn(Gp_ij, w_jc)), never contracted;
 *              an absent pair and j == i take part with Gp = 0 like any other term
 *   gp[i][c] = the chain over S = 0, 1, .. ascending, from +0.0, of acc = __dadd_rn(acc, b_S)
 * So the bits of a column do not depend on C, on the column's place in the batch, on the passes, the scheduling or the kernel mode,
 * and two calls give the same bytes.
 * The block terms b_S wait in device memory for the finishing kernel; they are bounded by a budget (2 GiB; GV_GRM_PART_MB, read by
 * gv_create).  The budget decides the edge g of the square tiles of g x g blocks the call walks the block triangle in, one pass per
 * tile: 2 sides x 3 operators x g^2 x 64 x C x 8 bytes fit in it.  Passes change no bit and compute no block twice; gv_grm_info
 * reports them.  A budget below the terms of one block (g = 1) is refused.
 *
 * gv_grm_he(ctx, use, C, y, res): Haseman-Elston regression (GCTA --HEreg) of C >= 1 traits, y N x C row-major on the host, NaN = missing.
 * Per trait: K = the individuals with a finite phenotype, n_K = |K|, m = sum y / n_K, v = sum (y - m)^2 / (n_K - 1),
 * yt = (y - m) / sqrt(v) on K and 0 elsewhere; the columns k (the indicator of K), yt and yt^2 go through gv_grm_apply, ten traits a
 * call.  The OLS regression of z = yt_i yt_j on x = A_ij over the pairs {i < j in K, M_ij > 0} follows from
 *   n = k'G0 k / 2   Sx = k'G1 k / 2   Sxx = k'G2 k / 2   Sz = yt'G0 yt / 2   Szz = (yt^2)'G0 (yt^2) / 2   Sxz = yt'G1 yt / 2
 *   D = n Sxx - Sx^2    h2 = (n Sxz - Sx Sz) / D    intercept = (Sz - h2 Sx) / n    RSS = Szz - intercept Sz - h2 Sxz
 *   se_ols = sqrt(RSS / (n - 2) * n / D)
 * all in fp64 on the host, O(N) per trait.  The delete-one-individual jackknife takes row i's terms u_i (G v)_i out of every sum for
 * i in K, keeps the standardisation of the full K, and gives se_jack = sqrt((n_K - 1) / n_K * sum (h2_(-i) - mean)^2).
 * h2, intercept, se_ols and se_jack are NaN when n < 3, D <= 0 or v is not a positive number (a constant trait, n_K < 2); the call
 * still returns 0.  A trait's result does not depend on the traits beside it.
 * Refused with a message, nothing written: everything gv_grm_block refuses; C out of range; NULL w, y or res; g0, g1 and g2 all NULL; a
 * w that is not finite; an infinite y; the budget case above. */
#define GV_GRM_APPLY_MAX_COLS 32
typedef struct gv_he_result {
    int64_t n_ind;               /* n_K */
    int64_t n_pairs;             /* n: the pairs of the regression */
    double sum_a, sum_aa;        /* Sx, Sxx over those pairs */
    double h2, intercept, se_ols, se_jack;
} gv_he_result;
int gv_grm_apply(gv_ctx* ctx, const uint8_t* use /* M or NULL */, int C, const double* w /* N x C */, double* g0, double* g1,
                 double* g2 /* N x C each, or NULL */);
int gv_grm_he(gv_ctx* ctx, const uint8_t* use /* M or NULL */, int64_t C, const double* y /* N x C */, gv_he_result* res /* C */);

/* ---- covariate-adjusted association screen: partial regression on the batch product (additions only: GV_ABI_VERSION stays 4; DESIGN.md
 * section 26) ------------------------------------------------------------------------------------------------------------------------
 * The regression of a phenotype y on [1, covariates, g_j] for every marker j, by the Frisch-Waugh-Lovell theorem: with Q an
 * orthonormal basis of the centred covariates and u the unit-norm residual of y, everything a marker needs is A^T u and A^T Q.
 * Data, mask and marker statistics are those of gv_screen_dev: 2-bit genotypes, alpha_scale == 1, n = nonas, a missing genotype counts
 * as the marker's mean.  xh_j = sqrt(N / (n - 1)) A_j is the unit-norm centred mean-imputed column of marker j (msig_j^2 sxx_j = n - 1).
 *
 * gv_screen_cov_set(ctx, K, cov): cov[k] are K raw covariate columns (N-space, not modified; values at NA and pad slots are ignored),
 * 0 <= K <= GV_PCA_MAX_BLOCK.  On the device, column k is zeroed outside the mask; centred, q <- q - fl(sum q / n) at the phenotyped; and
 * divided by fl(sqrt(sum q^2)); every sum in a fixed order that is a function of npad alone.  The panel is then orthonormalised by
 * CholeskyQR applied twice with the kernels and under the pivot rule of gv_pca_dev (32 * 2^-52 of the diagonal entry).  A column whose
 * sum of squares is not a positive finite number (constant over the phenotyped, or not finite there) and a pivot that is not positive
 * refuse the call: the covariates are collinear with each other or with the intercept, which is implicit (Q is orthogonal to the mask
 * vector because its columns are centred).  Then, with Z = gv_atxm_dev(Q) (M x K, scratch only) and c = fl(N / (n - 1)):
 *     s_j = sum_k z_jk^2     ascending k, s = fma(z, z, s) from 0
 *     v_j = fma(-c, s_j, 1)  the share of marker j's variance that the covariates leave; 1 / v_j is its variance-inflation factor
 * The context keeps Q (K columns of npad doubles), v (M doubles) and K in an allocation of its own, gv_screen_cov_stats.cached_bytes,
 * until gv_set_mask, gv_marker_stats, an upload or gv_set_dims drops them (the table above).  K == 0 is valid: an intercept only,
 * v == 1.  A refused call leaves the state cached before it as it was.  The call returns when its device work has finished.
 *
 * gv_screen_cov_dev(ctx, C, y, vif_max, r, t, p, beta, se): y[c] are C raw phenotype columns (N-space, not modified; values outside
 * the mask are ignored; a NaN inside the mask makes that column's outputs NaN and no other's).  C is processed in blocks of at most 32
 * columns.  On the device, per column: zeroed outside the mask and centred as a covariate is; projected twice,
 *     g_k = sum_n q_k[n] y[n] (the order of k_pca_gram)        y[n] <- fma(-q_k[n], g_k, y[n]) for k ascending
 * S = sum y^2 (fixed order), u = fl(y / fl(sqrt(S))).  With w = gv_atxm_dev(u), nu = n - 2 - K, per marker and column, in this order of
 * fp64 roundings:
 *     a    = fl(sqrt(fl(N / (n - 1))))                       (host, once)
 *     rho  = fl(fl(w a) / fl(sqrt(v_j)))                     the partial correlation              -> r
 *     om   = fma(-rho, rho, 1)
 *     t    = fl(rho fl(sqrt(fl(nu / om))))                   p = gvp::t_two_sided(|t|, nu)
 *     d    = fl(fl((n - 1) / fl(msig_j msig_j)) v_j)         sxx_j v_j
 *     beta = fl(rho fl(sqrt(fl(S / d))))                     per unit of the genotype value 0 / 1 / 2
 *     se   = fl(sqrt(fl(fl(S om) / fl(nu d))))
 * om <= 0 gives t = +-inf (the sign of rho), p = 0, se = 0.  NaN in all five outputs: a marker with sumsqx == 0 (the rule of
 * gv_screen_dev); a marker with v_j vif_max < 1 (the --vif rule of plink2 --glm; it bounds the cancellation in v_j); a column whose S is
 * not positive (the covariates explain the phenotype; accepted, not refused).  vif_max is finite and >= 1.
 * r is required; t, p, beta and se may be NULL arrays.  All outputs are distinct M-space vectors.
 * Column independence: the outputs of a column are bit-identical whatever C is, wherever the column stands and whatever the other
 * columns hold: the batch product guarantees it, a Gram entry's summation order is a function of npad alone, and every other step is
 * per column.
 * Refused with a message, nothing written: everything gv_screen_dev refuses; K < 0 or K > GV_PCA_MAX_BLOCK; nu < 1; NULL arrays or
 * handles, vectors of the wrong space, of another context or of earlier dimensions; two outputs that are the same vector; vif_max that is
 * NaN, infinite or < 1; collinear covariates; gv_screen_cov_dev before gv_screen_cov_set, or after its state was dropped (the message
 * names gv_screen_cov_set).
 * Work panels: gv_pca_dev's scratch, owned by the context, grown on demand.  The calls leave the context as they found it, by the rule
 * of gv_atxm_dev / gv_pca_dev.  Both return when their device work has finished (the seconds below are device events).
 * A context joined to others (a marker-sharded job): neither call issues a collective.  The basis Q and the residual columns are
 * N-space and computed by every rank for itself, in an order that depends on npad alone, so they are the same bits on every rank that
 * was given the same covariates, columns and mask; v_j and the five outputs are quantities of one marker.  The outputs of the ranks,
 * side by side in marker order, are the outputs of one context on all markers bit for bit.  Both calls succeed on a rank without
 * markers. */
typedef struct gv_screen_cov_stats {
    int K;                       /* covariates of the cached state; -1: none cached */
    int pad_;
    int64_t nu;                  /* n - 2 - K of the cached state (0 when none) */
    uint64_t cached_bytes;       /* bytes of Q and v the context holds */
    double set_seconds_products; /* last successful gv_screen_cov_set: device time in the batch product */
    double set_seconds_panel;    /* ... in the panel kernels: masking, centring, scaling, CholeskyQR, v */
    double set_seconds;          /* ... host wall time of the call */
    int64_t columns;             /* last gv_screen_cov_dev: C */
    double call_seconds_products; /* ... device time in the batch product */
    double call_seconds_panel;   /* ... in the panel and finishing kernels */
    double call_seconds;         /* ... host wall time of the call */
} gv_screen_cov_stats;
int gv_screen_cov_set(gv_ctx* ctx, int K, const gv_vec* const* cov /* K, GV_SPACE_N, not modified */);
int gv_screen_cov_dev(gv_ctx* ctx, int64_t C, const gv_vec* const* y /* C, GV_SPACE_N, not modified */, double vif_max,
                      gv_vec* const* r, gv_vec* const* t, gv_vec* const* p, gv_vec* const* beta,
                      gv_vec* const* se /* C each, GV_SPACE_M; all but r may be NULL arrays */);
int gv_screen_cov_info(const gv_ctx* ctx, gv_screen_cov_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* GVAMP_H */
