// data.hpp -- host side of the reference's `class data` (data.hpp:18-146) for the linear model: same constructors,
// getters and Ax / ATx signatures; the genotype block lives in HBM behind a gv_ctx and every matvec is a HIP kernel
// (include/gvamp.h).  No CPU path: construction fails (exit, as the reference does on I/O errors) without a GPU.
#pragma once
#include <string>
#include <vector>

#include "gvamp.h"

// the process's one communicator (RCCL, or the shared-memory host transport with GVAMP_COMM=host), created at first use by the
// first data object of a sharded run; gv_host_finalize() is the drivers' MPI_Finalize
gv_ctx* gv_host_world(int device);
void gv_host_finalize();

class data {
private:
    std::string phenfp, bedfp, methfp, bimfp, type_data = "bed";
    int N = 0, M = 0, Mt = 0, S = 0, rank = 0;
    int nonas = 0, nas = 0, im4 = 0;
    size_t mbytes = 0;
    std::vector<double> phen_data;
    std::vector<unsigned char> mask4;
    std::vector<double> mave, msig;    // host copies of the device statistics (get_mave / get_msig)
    std::vector<std::vector<double>> covs;
    double intercept = 0, scale = 1, alpha_scale = 1;
    double dosage_scale = 0;           // [ext] type_data "dosage8" / "dosage16": value = scale * code; <= 0 = 1/127, 1/16384
    int dosage_missing = 0;            // [ext] ... 1: the all-ones code is a missing entry (gv_set_dosage_missing)
    int dosage_route = 0;              // [ext] ... 1: the products on the fixed-point i8 MFMA route where it applies (gv_set_dosage_route)
    gv_ctx* ctx = nullptr;
    bool owns_ctx = true;

    void open_device(int device, int kernel_mode);
    void push_mask();

public:
    // data.cpp:69-113 -- phenotype given as a vector, every individual present
    data(std::vector<double> y, std::string genofp, const int N, const int M, const int Mt, const int S, const int rank,
         std::string type_data = "bed", double alpha_scale = 1, std::string bimfp = "", int device = -1,
         int kernel_mode = 1, double dosage_scale = 0, int dosage_missing = 0, int dosage_route = 0);
    // data.cpp:30-61 -- phenotype file (.phen) with NA handling
    data(std::string fp, std::string genofp, const int N, const int M, const int Mt, const int S, const int rank,
         std::string type_data = "bed", double alpha_scale = 1, std::string bimfp = "", int device = -1,
         int kernel_mode = 1, double dosage_scale = 0, int dosage_missing = 0, int dosage_route = 0);
    // [ext] adopt a context whose genotype shard is already resident (synthetic shards, bench, tests).
    // The context's mask is replaced by the full mask unless mask4 is given.
    data(gv_ctx* resident, std::vector<double> y, const int N, const int M, const int Mt, const int S, const int rank,
         const std::vector<unsigned char>* mask4 = nullptr, int nonas = -1, double alpha_scale = 1);
    ~data();
    data(const data&) = delete;
    data& operator=(const data&) = delete;

    std::vector<double> get_phen() { return phen_data; }
    void set_phen(std::vector<double> new_data) { phen_data = new_data; }
    std::string get_bimfp() { return bimfp; }
    double get_intercept() { return intercept; }
    double get_scale() { return scale; }
    size_t get_mbytes() { return mbytes; }
    double* get_mave() { return mave.data(); }
    double* get_msig() { return msig.data(); }
    std::vector<unsigned char>& get_mask4() { return mask4; }
    int get_im4() const { return im4; }
    int get_nonas() { return nonas; }
    void set_nonas(int num) { nonas = num; }
    int get_S() const { return S; }
    int get_N() const { return N; }
    int get_M() const { return M; }
    int get_Mt() const { return Mt; }
    std::string get_type_data() const { return type_data; }
    gv_ctx* get_ctx() { return ctx; }

    void read_phen();                       // data.cpp:128-192
    void read_genotype_data();              // data.cpp:201-234
    void read_methylation_data();           // data.cpp:241-278 (type_data == "meth")
    void read_dosage_data();                // [ext] type_data == "dosage8" / "dosage16": 8- / 16-bit dosage codes
    std::vector<int> read_chromosome_info(std::string bim_file);   // data.cpp:346-380
    void compute_markers_statistics();      // data.cpp:392-546
    // [ext] many weight vectors in one pass over the genotypes (gv_score): column j = Ax(cols[j]), bit for bit
    std::vector<std::vector<double>> score(const std::vector<std::vector<double>>& cols);
    // [ext] many phenotype vectors in one pass over the genotypes (gv_atxm): column j = ATx(cols[j]), bit for bit;
    // cols[j] holds 4 * mbytes doubles
    std::vector<std::vector<double>> ATx_multi(const std::vector<std::vector<double>>& cols);
    // [ext] the marginal association screen (gv_screen_dev): cols[j] = N raw phenotype values, NaN for NA, every NA outside the mask.
    // Returns {r, t, p}, each C columns of M values.
    std::vector<std::vector<std::vector<double>>> screen(const std::vector<std::vector<double>>& cols);
    // [ext] the covariate-adjusted screen (gv_screen_cov_set / gv_screen_cov_dev).  screen_cov_set: the K columns
    // of the covariates read_covariates / set_covs left (N rows of K values; none: the intercept alone) become the context's cached
    // basis.  screen_cov: cols[j] = N raw phenotype values, used as they are (values outside the mask are ignored).  Returns
    // {r, t, p, beta, se}, each C columns of M values.
    void screen_cov_set();
    std::vector<std::vector<std::vector<double>>> screen_cov(const std::vector<std::vector<double>>& cols, double vif_max);
    // [ext] principal components of the resident genotypes (gv_pca_dev): the k leading eigenpairs of the
    // relationship matrix from a starting block of L columns of pca_start(seed, ...); loadings: this shard's M values per component
    struct pca_result {
        std::vector<double> eval, resid;
        std::vector<std::vector<double>> evec, loadings;      // k x 4 * mbytes, k x M (empty without loadings)
        gv_pca_stats info;
    };
    pca_result pca(int k, int L, double tol, int max_iter, unsigned long long seed, bool loadings);
    // entry n of column j of the starting block: Box-Muller on two splitmix64 outputs of the counter 2 (j N + n) (+ 1) from `seed`
    static double pca_start(unsigned long long seed, unsigned long long index);
    // [ext] pairwise kinship of the resident genotypes (gv_king_pairs / gv_king_block).  use: M bytes, non-zero = the
    // marker counts (empty: every marker).  king_pairs: every pair i < j with kin >= cutoff in ascending (i, j), re-called once with the
    // number found when the first call's slots did not suffice; king_block: the rectangle [i0, i0 + ni) x [j0, j0 + nj), row-major
    struct king_result {
        std::vector<int32_t> i, j;          // king_pairs only
        std::vector<double> kin;
        std::vector<int32_t> counts;        // 5 per entry: nsnp, hethet, ibs0, het_i, het_j
        gv_king_stats info;
    };
    king_result king_pairs(double cutoff, const std::vector<unsigned char>& use = std::vector<unsigned char>());
    king_result king_block(int64_t i0, int64_t ni, int64_t j0, int64_t nj, const std::vector<unsigned char>& use = std::vector<unsigned char>());
    // [ext] the standardised genetic relationship matrix of the resident genotypes (gv_grm_pairs / gv_grm_block).
    // use as above.  grm_pairs: every pair i < j with A_ij >= cutoff in ascending (i, j) and the N diagonal entries, re-called once with
    // the number found when the first call's slots did not suffice; grm_block: the rectangle [i0, i0 + ni) x [j0, j0 + nj), row-major
    struct grm_result {
        std::vector<int32_t> i, j;          // grm_pairs only
        std::vector<double> a;
        std::vector<int32_t> m_common;
        std::vector<double> diag;           // grm_pairs only: A_ii
        std::vector<int32_t> diag_m;        // grm_pairs only: M_ii
        gv_grm_stats info;
    };
    grm_result grm_pairs(double cutoff, const std::vector<unsigned char>& use = std::vector<unsigned char>());
    grm_result grm_block(int64_t i0, int64_t ni, int64_t j0, int64_t nj, const std::vector<unsigned char>& use = std::vector<unsigned char>());
    // [ext] the GRM-times-panel product and Haseman-Elston regression on it (gv_grm_apply / gv_grm_he).  w and y
    // are N x C row-major (a NaN in y: the phenotype is missing); grm_apply returns g0, g1, g2, N x C each
    struct grm_apply_result {
        std::vector<double> g0, g1, g2;
        gv_grm_stats info;
    };
    struct grm_he_result {
        std::vector<gv_he_result> traits;
        gv_grm_stats info;
    };
    grm_apply_result grm_apply(int C, const std::vector<double>& w, const std::vector<unsigned char>& use = std::vector<unsigned char>());
    grm_he_result grm_he(int64_t C, const std::vector<double>& y, const std::vector<unsigned char>& use = std::vector<unsigned char>());
    // [ext] replace the mask (bit n & 3 of byte n >> 2 set: individual n has a phenotype) and recompute the marker statistics
    void set_mask(const std::vector<unsigned char>& m4, int nonas_);
    std::vector<double> Ax(double* __restrict__ phen);    // data.cpp:848 : M doubles -> 4*mbytes, reduced + scaled
    std::vector<double> ATx(double* __restrict__ phen);   // data.cpp:810 : 4*mbytes doubles -> M
    // covariates of the probit model (data.cpp:286-331, :1050-1058): one row of C values per individual
    void read_covariates(std::string covfp, int C = 0);
    std::vector<std::vector<double>> get_covs() { return covs; }
    void set_covs(std::vector<std::vector<double>> z) { covs = std::move(z); }   // [ext] covariates given in memory
    std::vector<double> Zx(std::vector<double> phen);     // 4*mbytes: <covs[i], phen> for i < N, 0 beyond
    std::vector<double> filter_pheno();                   // data.cpp:1065-1079
    std::vector<double> filter_pheno(int* nonnan);        // data.cpp:1081-1097
    // data.cpp:1108-1226 / :1235-1353 -- leave-one-out / leave-one-chromosome-out t-test p-values, one vector per
    // estimator; written to filepath[ie] (LOO) or filepath[ie] + "_pvals_LOCO.bin" (LOCO) at byte offset S*8.
    std::vector<std::vector<double>> pvals_calc(std::vector<std::vector<double>> z1, std::vector<double> y,
                                                std::vector<std::vector<double>> x1_hat, std::vector<std::string> filepath);
    std::vector<std::vector<double>> pvals_calc_LOCO(std::vector<std::vector<double>> z1, std::vector<double> y,
                                                     std::vector<std::vector<double>> x1_hat,
                                                     std::vector<std::string> filepath);
    // the same on device handles (what vamp::infere_linear calls): z1, y N-space; x1_hat M-space
    // pred_prefix (LOCO only, may be empty): also dump the per-chromosome predictors <prefix>_LOCO_chr_<ch>.csv (data.cpp:1276-1281)
    std::vector<double> pvals_calc_dev(gv_vec* z1, gv_vec* y, gv_vec* x1_hat, bool loco, const std::string& pred_prefix = std::string());
    // [ext] the whole test of gv_assoc_loo / gv_assoc_loco: {beta, se, t, p}, M values each (bed and compact dosage data)
    std::vector<std::vector<double>> assoc_calc_dev(gv_vec* z1, gv_vec* y, gv_vec* x1_hat, bool loco, const std::string& pred_prefix = std::string());
    // [ext] gv_ld_scores over `window` markers on each side: {l2, npairs}, M values each; per chromosome when a .bim file was given
    std::vector<std::vector<double>> ld_scores_dev(int window, bool adjusted);
    // [ext] the positions of this shard's markers from a .bim file: unit "cm" = column 3, "bp" = column 4
    std::vector<double> read_positions(std::string bim_file, const std::string& unit);
    // [ext] an annotation file: one header line, then one row per marker in marker order, M rows; the columns headed CHR, BP, SNP or CM
    // are skipped, every other column is a category.  Returns M x C row-major and the C names.
    std::vector<double> read_annot(std::string path, int M, std::vector<std::string>* names);
    // [ext] gv_ld_scores_pos: {l2 (M x max(ncat, 1) row-major), npairs (M)}; annot empty = no annotation; per chromosome when a .bim
    // file was given
    // [ext] gv_ld_clump: index_of of every marker (local indices, -1 = in no clump) and the number of index
    // markers; per chromosome when a .bim file was given
    std::vector<int64_t> ld_clump_dev(const std::vector<double>& pos, double radius, const std::vector<double>& p, double p1, double p2,
                                      double r2, int64_t* n_index);
    std::vector<std::vector<double>> ld_scores_pos_dev(const std::vector<double>& pos, double radius, bool adjusted,
                                                       const std::vector<double>& annot, int ncat);
};
