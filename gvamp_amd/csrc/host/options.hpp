// options.hpp -- `class Options`: the command line of the reference (options.hpp:5-155, options.cpp:18-429),
// same flag spellings, defaults, getter names and fatal-error behaviour.  One table (GV_OPTION_FIELDS) declares every
// scalar option -- type, member, default -- and generates the member and its `get_<member>()`; the parser in options.cpp
// is table-driven too (the reference has a strcmp chain and hand-written getters).  Extensions of this build: [ext].
#pragma once
#include <string>
#include <vector>

// X(type, member, default)
#define GV_OPTION_FIELDS(X)                                                                                          \
    /* files and run selection */                                                                                    \
    X(std::string, bed_file, "") X(std::string, bed_file_test, "") X(std::string, bim_file, "")                     \
    X(std::string, estimate_file, "") X(std::string, cov_estimate_file, "") X(std::string, cov_file, "")           \
    X(std::string, freeze_index_file, "") X(std::string, out_dir, "") X(std::string, out_name, "")                 \
    X(std::string, model, "linear") X(std::string, run_mode, "")                                                    \
    /* problem sizes (uninitialised in the reference) */                                                             \
    X(unsigned int, N, 0) X(unsigned int, Mt, 0) X(unsigned int, N_test, 0) X(unsigned int, Mt_test, 0)              \
    X(unsigned int, num_mix_comp, 0) X(unsigned int, C, 0) X(unsigned int, CV, 0)                                     \
    /* solver (options.hpp:107-...) */                                                                                \
    X(unsigned int, iterations, 1) X(unsigned int, EM_max_iter, 2) X(unsigned int, CG_max_iter, 60)                   \
    X(double, stop_criteria_thr, 1e-4) X(double, EM_err_thr, 1e-2) X(double, rho, 0.15) X(double, h2, -1)            \
    X(double, probit_var, 1) X(double, alpha_scale, 1.0) X(double, gamw_init, 0) X(double, gam1_init, -1)            \
    X(double, gamma_damp, 1)                                                                                          \
    X(unsigned int, learn_vars, 1) X(unsigned int, seed, 1) X(unsigned int, init_est, 0) X(unsigned int, redglob, 0) \
    X(unsigned int, use_lmmse_damp, 0) X(unsigned int, use_XXT_denoiser, 0) X(unsigned int, use_freeze, 0)            \
    X(unsigned int, store_pvals, 0)                                                                                   \
    /* [ext] --device (default: LOCAL_RANK or 0), --kernel-mode 0|1|2 (default 1: i8 MFMA; 2: the same in two-level fixed point), --synth-seed S (on-device   \
       synthetic .bed when there is no --bed-file), --synth-miss-ppm, --diagnostics 1 (the 3 print-only Ax of         \
       vamp.cpp:646-681), --store-iterates 0 (skip the per-iteration .bin/.csv dumps), --fuse-solves (default 4): 0 the reference\
       sequence; 1 the LMMSE and Onsager CG solves share their passes (bit-identical); 2 also z1 = A x1_hat rides in  \
       a free slot and A x2_hat, A^T A invQ u come out of the CG recurrences (rounding-level); 3 also the warm start's \
       initial residual comes from the previous solve's final residual (no pass); 4 also the Onsager solve's first  \
       step comes from A^T A u of the probe, computed once (rounding-level, like 2 and 3); --resident-layout 1|2|3:    \
       kernel mode 1 keeps two stripe sets (2 x M N / 4 bytes) or one tile layout (M N / 4 bytes) in HBM, same bits; \
       3 (default) = two stripe sets if they fit the free HBM, else the tile layout; --reanchor-every K (default 10, 0 =  \
       never): at --fuse-solves 3 / 4 every K-th iteration applies the operator to the warm start explicitly and captures \
       A^T A u afresh, so the products chained from CG residuals never run unanchored for more than K iterations;    \
       --huber-delta-schedule deferred|reference (--model robust): deferred (default) moves       \
       iteration 1's delta_H step to the start of iteration 2's z side, reference keeps vamp_Huber.cpp's order;       \
       --cg-precond scalar|ld (default scalar) and --cg-precond-window 32|64|128 (default 128): the preconditioner of   \
       the M-space CG solves, ld = two grids of LD-block windows;                                \
       --geno-format bed|dosage8|dosage16 (default bed): what --bed-file / --bed-file-test hold -- PLINK rows, or a     \
       marker-major matrix of 8- / 16-bit dosage codes;                                         \
       --dosage-scale s: value = s * code (default 1/127 for dosage8, 1/16384 for dosage16);                            \
       --dosage-missing 0|1 (default 0): 1 = the all-ones code (255 / 65535) is a missing entry (gv_set_dosage_missing); \
       ignored with one warning line for --geno-format bed;                                                            \
       --dosage-kernels valu|mfma (default valu): the products of dosage8 codes on the fp64 VALU kernels or on the        \
       fixed-point i8 MFMA route (gv_set_dosage_route; in force for 8-bit codes without missing entries, the line         \
       "dosage kernels: ..." names what runs); ignored with one warning line for --geno-format bed;                      \
       --store-assoc 0|1 (default 0): after the loop write the whole per-marker association test -- effect, standard  \
       error, t and p, LOO and (with a .bim file) LOCO -- for bed and dosage data;              \
       --run-mode ldscore with --ld-window B (1..8192, default 200) and --ld-adjust 0|1 (default 0): the LD scores of    \
       the markers over B markers on each side, per chromosome with a .bim file;                \
       --ld-dosage 0|1 (default 0): 1 = --run-mode ldscore also accepts --geno-format dosage8 (gv_set_ld_dosage,         \
       DESIGN.md section 17; with --dosage-missing 1 the code 255 is a missing entry), and --cg-precond ld accepts it   \
       in the infere / restart / both modes (section 18);                                                              \
       --ld-wind-kb X / --ld-wind-cm X (instead of --ld-window; need --bim-file): the window of --run-mode ldscore by    \
       distance, X kb of the .bim file's base-pair column (radius 1000 X) or X cM of its cM column, at most 8192 markers \
       ahead (gv_ld_scores_pos); --ld-annot FILE: one header line, one row per marker, the columns \
       CHR / BP / SNP / CM skipped and every other column an annotation category -- partitioned LD scores, M x C, with    \
       <out>_ldscore_M.txt (the category sums over the polymorphic markers and over those of MAF > 0.05) and            \
       <out>_ldscore_cats.txt (the names); without a kb / cM window the positions are the marker indices;              \
       --run-mode clump (gv_ld_clump) with --clump-p-file FILE (Mt raw float64, the format of      \
       <out>_assoc_p.bin), --clump-p1 (default 1e-4: index markers), --clump-p2 (default 1e-2: members), --clump-r2      \
       (default 0.5) and exactly one window: --clump-kb X (default 250; needs --bim-file), --ld-wind-cm X or --ld-window B \
       -- LD clumping of association results: <out>_clump_index.bin and <out>_clumps.txt;                               \
       --run-mode score (gv_score) with --bed-file-test / --N-test / --Mt-test, --score-file FILE   \
       (raw float64, C x Mt values, column after column) and --score-cols C (default 1): <out>_scores.bin, C columns of  \
       N float64; --score-units std|allele (default std: a column is effects per standardised genotype, scaled by       \
       sqrt(N) as predict scales them; allele: weights per copy of the .bim file's first allele, a missing genotype      \
       counts as the marker's mean); --score-clump-index FILE --score-p-file FILE --score-p-thresholds t1,t2,...:        \
       clumping and thresholding, column k = column 0 at the index markers with p <= t_k (needs --score-cols 1);        \
       --run-mode screen (gv_screen_dev) with --phen-files f0,f1,...: the marginal association      \
       screen of every phenotype file against every marker over the complete cases (an individual with NA in any file    \
       is masked): <out>_screen_{r,t,p}.bin, one column of Mt float64 per file; --screen-cols K (default 64): columns    \
       per call; with --cov-file F --C K (gv_screen_cov_set / gv_screen_cov_dev; F holds N lines    \
       of K numbers, the format of <out>_pca_eigenvec.txt) the screen is adjusted for the K covariates and an            \
       intercept: an individual with a non-finite covariate is masked together with the NA phenotypes, a marker whose     \
       variance-inflation factor given the covariates is above --screen-vif (default 50) gets NaN, and                    \
       <out>_screen_{beta,se}.bin (per copy of the counted allele) are written beside the three files;                    \
       --screen-dosage 0|1 (default 0): 1 = --run-mode screen also accepts --geno-format dosage8 / dosage16                 \
       (gv_set_screen_dosage, DESIGN.md section 29: the mean-imputed dosage, beta per unit of scale * code), with          \
       --dosage-scale, --dosage-missing and --dosage-kernels as in the other modes; ignored with one warning line for     \
       --geno-format bed;                                                                                                 \
       --run-mode pca (gv_pca_dev) with --pca-k K: the K leading principal components of the       \
       standardised genotypes among the individuals with a phenotype, by block subspace iteration on a block of          \
       --pca-block L vectors (default min(32, K + max(8, K))) to --pca-tol t (default 1e-8) within --pca-max-iter n       \
       (default 100) iterations from the starting block of --pca-seed s (default 0); a run that misses the tolerance      \
       writes nothing and exits non-zero unless --pca-allow-unconverged 1 (default 0): <out>_pca_eigenval.txt,            \
       <out>_pca_eigenvec.txt (N lines of K numbers: a --cov-file for --C K) and <out>_pca_loadings.bin (K columns of    \
       Mt float64: a --score-file for --score-cols K);                                                                   \
       --run-mode king (gv_king_pairs) with --king-cutoff x (default 0.0884, second degree):        \
       every pair of individuals whose KING-robust kinship is at least x, from the bed file alone (no phenotype file),    \
       over the markers of --king-marker-file F (Mt bytes of 0 / 1; default: every marker): <out>_king.kin0.txt, one     \
       line "i j nsnp hethet ibs0 het_i het_j kinship" per pair in ascending (i, j);                                     \
       --run-mode grm (gv_grm_pairs / gv_grm_block): the standardised genetic relationship matrix  \
       A = Z Z^T / M_ij of GCTA from the bed file alone, over the markers of --grm-marker-file F (Mt bytes of 0 / 1;     \
       default: every marker).  With --grm-cutoff x: <out>.grm.sp, GCTA's sparse text, "i j value" with 0-based          \
       indices, the N diagonal entries first and then every pair with A_ij >= x in ascending (i, j).  Without it:        \
       <out>.grm.bin (the lower triangle with the diagonal, row by row, float32) and <out>.grm.N.bin (the common-marker  \
       counts in the same order, float32), GCTA's dense format;                                                          \
       --run-mode he (gv_grm_he) with --phen-files f0,f1,... [--grm-marker-file F]: Haseman-Elston   \
       regression (GCTA --HEreg) of every phenotype file on that matrix, which is never stored; every trait keeps its     \
       own missing (NA) individuals: <out>.HEreg, a header line and one line per file, "trait n_ind n_pairs mean_a var_a  \
       h2 intercept se_ols se_jack" */                                                       \
    X(int, device, -1) X(int, kernel_mode, 1) X(long, synth_seed, -1) X(unsigned int, synth_miss_ppm, 5000)          \
    X(int, diagnostics, 0) X(int, store_iterates, 1) X(int, fuse_solves, 4) X(int, resident_layout, 3)              \
    X(int, reanchor_every, 10) X(std::string, huber_delta_schedule, "deferred") X(std::string, cg_precond, "scalar")    \
    X(int, cg_precond_window, 128) X(std::string, geno_format, "bed") X(double, dosage_scale, 0) \
    X(unsigned int, store_assoc, 0) X(int, dosage_missing, 0) X(std::string, dosage_kernels, "valu")       \
    X(int, ld_window, 200) X(int, ld_adjust, 0) X(int, ld_dosage, 0)                                                   \
    X(double, ld_wind_kb, -1) X(double, ld_wind_cm, -1) X(std::string, ld_annot, "")                                   \
    X(std::string, clump_p_file, "") X(double, clump_p1, 1e-4) X(double, clump_p2, 1e-2) X(double, clump_r2, 0.5)      \
    X(double, clump_kb, -1)                                                                                          \
    X(std::string, score_file, "") X(unsigned int, score_cols, 1) X(std::string, score_units, "std")                \
    X(std::string, score_clump_index, "") X(std::string, score_p_file, "") X(unsigned int, screen_cols, 64)   \
    X(double, screen_vif, 50.0) X(int, screen_dosage, 0)                                                             \
    X(unsigned int, pca_k, 0) X(unsigned int, pca_block, 0) X(double, pca_tol, 1e-8) X(unsigned int, pca_max_iter, 100)          \
    X(unsigned int, pca_seed, 0) X(unsigned int, pca_allow_unconverged, 0)                                           \
    X(double, king_cutoff, 0.0884) X(std::string, king_marker_file, "")                                              \
    X(double, grm_cutoff, 0.0) X(int, grm_has_cutoff, 0) X(std::string, grm_marker_file, "")

class Options {
public:
    Options() = default;
    Options(int argc, char** argv) {
        read_command_line_options(argc, argv);
        check_options();
    }
    void read_command_line_options(int argc, char** argv);

#define GV_X(T, n, d) T get_##n() const { return n; }
    GV_OPTION_FIELDS(GV_X)
#undef GV_X
    // list-valued options
    std::vector<double> get_vars() const { return vars; }
    std::vector<double> get_probs() const { return probs; }
    std::vector<int> get_test_iter_range() const { return test_iter_range; }
    const std::vector<std::string>& get_phen_files() const { return phen_files; }
    const std::vector<std::string>& get_phen_files_test() const { return phen_files_test; }
    const std::vector<std::string>& get_true_signal_files() const { return true_signal_files; }
    int count_phen_files() const { return (int)phen_files.size(); }
    int count_phen_files_test() const { return (int)phen_files_test.size(); }
    const std::vector<double>& get_score_p_thresholds() const { return score_p_thresholds; }      // [ext] --score-p-thresholds
    int count_ld_windows() const { return ld_windows_given; }      // [ext] how many of --ld-window / --ld-wind-kb / --ld-wind-cm were given
    void list_phen_files() const;

    void set_probit_var(double v) { probit_var = v; }
    // [ext] programmatic construction (host_capi.cpp): the solver knobs that `vamp` reads through the getters above
    void set_solver(unsigned int EM_max_iter_, unsigned int CG_max_iter_, double EM_err_thr_, double stop_criteria_thr_,
                    unsigned int learn_vars_, unsigned int seed_, unsigned int use_lmmse_damp_, int diagnostics_,
                    int store_iterates_) {
        EM_max_iter = EM_max_iter_; CG_max_iter = CG_max_iter_; EM_err_thr = EM_err_thr_;
        stop_criteria_thr = stop_criteria_thr_; learn_vars = learn_vars_; seed = seed_;
        use_lmmse_damp = use_lmmse_damp_; diagnostics = diagnostics_; store_iterates = store_iterates_;
    }
    void set_use_XXT_denoiser(unsigned int v) { use_XXT_denoiser = v; }
    void set_fuse_solves(int v) { fuse_solves = v; }
    void set_reanchor_every(int v) { reanchor_every = v; }
    void set_huber_delta_schedule(const std::string& v) { huber_delta_schedule = v; }
    void set_cg_precond(const std::string& v, int window) { cg_precond = v; cg_precond_window = window; }
    void set_C(unsigned int v) { C = v; }
    void set_freeze(const std::string& file) { use_freeze = 1; freeze_index_file = file; }

private:
#define GV_X(T, n, d) T n = d;
    GV_OPTION_FIELDS(GV_X)
#undef GV_X
    std::vector<double> vars, probs;
    std::vector<int> test_iter_range = std::vector<int>(2, -1);
    std::vector<std::string> phen_files, phen_files_test, true_signal_files;
    int ld_windows_given = 0;
    std::vector<double> score_p_thresholds;

    void fail_if_last(char** argv, const int i);
    void check_options();
};
