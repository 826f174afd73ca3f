// score_cols.hpp -- the weight columns of a scoring batch (data::score / gv_score), built on the host.  Host-only and header-only:
// tests/test_score_cpu.py compiles it into a stand-alone program and holds it to tests/score_restatement.py.
//
// Units of a column.
//   std     the column is an x of data::Ax: effects per unit of the standardised genotype times sqrt(N) (the convention of `predict`).
//   allele  the column holds weights w per copy of the counted allele (a = 2 for PLINK code 00, the .bim file's first allele); a missing
//           genotype counts as the marker's mean (PLINK's default mean imputation for --score).  Then
//               S_n = sum_j w_j a~_nj = Ax(x)_n + K,   x_j = w_j sqrt(N) / msig_j,   K = sum_j mave_j w_j
//           because Ax(x)_n = sum_j (a~_nj - mave_j) msig_j x_j / sqrt(N) with a~ = mave at a missing genotype.  msig is never 0: a
//           monomorphic or all-missing marker has msig = 1 and contributes its constant mave_j w_j alone (a~ - mave = 0 there).
// Roundings, stated so that they can be restated: x_j = fl(fl(w_j * sqrtN) / msig_j); K is accumulated in marker order with ONE
// rounding per marker, K <- fma(mave_j, w_j, K), starting from 0.
//
// Clumping and thresholding: column k of the batch is column 0 of the score file at the index markers of the clumps
// (index_of[j] == j) whose p-value is at most threshold k (p_j <= t_k; a NaN p_j is in no column), and zero elsewhere.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace score_cols {

// allele-unit weights -> the x of data::Ax
inline std::vector<double> allele_to_std(const double* w, const double* msig, size_t M, double sqrtN) {
    std::vector<double> x(M);
    for (size_t j = 0; j < M; j++) {
        const double t = w[j] * sqrtN;
        x[j] = t / msig[j];
    }
    return x;
}

// the constant K of an allele-unit column
inline double allele_constant(const double* w, const double* mave, size_t M) {
    double k = 0.0;
    for (size_t j = 0; j < M; j++) k = std::fma(mave[j], w[j], k);
    return k;
}

// one column per threshold
inline std::vector<std::vector<double>> threshold_columns(const double* w0, const int64_t* index_of, const double* p, size_t M,
                                                          const std::vector<double>& thresholds) {
    std::vector<std::vector<double>> cols(thresholds.size(), std::vector<double>(M, 0.0));
    for (size_t k = 0; k < thresholds.size(); k++)
        for (size_t j = 0; j < M; j++)
            if (index_of[j] == (int64_t)j && p[j] <= thresholds[k]) cols[k][j] = w0[j];
    return cols;
}

}  // namespace score_cols
