// gv_ld_window.h -- the host side of a positional LD window (gv_ld_scores_pos): from the markers' positions and
// chromosomes to the last in-band index hi[j] of every marker.  No HIP in here: gv_ld.hip and a plain g++ program include it alike.
//
// k is in the band of j iff chrom_j == chrom_k and |pos_k - pos_j| <= radius, the comparison being the fp64 expression
// pos_k - pos_j <= radius for j <= k (equal positions are always in each other's band).  With pos finite and non-decreasing inside every
// maximal run of equal chrom and every chromosome id a single run, the band of j is the index interval [lo_j, hi_j], lo and hi do not
// decrease (fp64 subtraction and comparison are monotone), and k <= hi_j <=> j >= lo_k: the kernel needs hi alone.
#pragma once
#include <cmath>
#include <cstdint>
#include <unordered_set>
#include <vector>

namespace gvw {

enum Verdict {
    OK = 0,
    POS_NOT_FINITE,     // pos[at] is NaN or infinite
    POS_DECREASES,      // pos[at] < pos[at - 1] inside a run of one chromosome
    CHROM_REAPPEARS,    // chrom[at] starts a second run of an id whose run has ended
    REACH_TOO_LONG      // hi[at] - at = reach > max_reach
};

struct Window {
    std::vector<int64_t> hi;    // M: the last index in the band of j, the chromosome folded in
    int64_t dmax = 0;           // the most row groups a 64-marker row group I reaches ahead: max of hi[min(64 I + 63, M - 1)] / 64 - I
    double entries = 0.0;       // sum of hi_j - lo_j + 1 = M + 2 sum (hi_j - j), by the symmetry above
    Verdict verdict = OK;
    int64_t at = -1;            // the first offending marker
    int64_t reach = 0;          // REACH_TOO_LONG: its reach
};

// O(M): one pass over the input for the conditions, one two-pointer pass for hi.  chrom may be NULL (one chromosome); radius must be
// finite and >= 0 (the caller's check).
inline Window make_window(const double* pos, const int* chrom, double radius, int64_t M, int64_t max_reach) {
    Window w;
    std::unordered_set<int> ended;
    for (int64_t j = 0; j < M; j++) {
        const bool first = j == 0 || (chrom && chrom[j] != chrom[j - 1]);
        Verdict v = OK;
        if (!std::isfinite(pos[j])) v = POS_NOT_FINITE;
        else if (first && j > 0 && ended.count(chrom[j])) v = CHROM_REAPPEARS;
        else if (!first && pos[j] < pos[j - 1]) v = POS_DECREASES;
        if (v != OK) {
            w.verdict = v;
            w.at = j;
            return w;
        }
        if (first && j > 0) ended.insert(chrom[j - 1]);
    }
    w.hi.resize((size_t)M);
    int64_t k = 0, over = 0;
    for (int64_t j = 0; j < M; j++) {
        if (k < j) k = j;
        while (k + 1 < M && (!chrom || chrom[k + 1] == chrom[j]) && pos[k + 1] - pos[j] <= radius) k++;
        if (k - j > max_reach) {
            w.verdict = REACH_TOO_LONG;
            w.at = j;
            w.reach = k - j;
            w.hi.clear();
            return w;
        }
        w.hi[(size_t)j] = k;
        over += k - j;
    }
    w.entries = (double)M + 2.0 * (double)over;
    for (int64_t I = 0; I * 64 < M; I++) {
        const int64_t last = I * 64 + 63 < M - 1 ? I * 64 + 63 : M - 1;
        const int64_t d = w.hi[(size_t)last] / 64 - I;
        if (d > w.dmax) w.dmax = d;
    }
    return w;
}

}  // namespace gvw
