// gv_ld_clump.h -- the host side of LD clumping (gv_ld_clump): from the p-values and the positional window
// (gv_ld_window.h) to the order of the eligible markers, the two eligibility sets and the list of blocks the block kernel is launched
// on.  No HIP in here: gv_ld.hip and a plain g++ program include it alike.
//
// E2 = { j : p_j <= p2 } may be a member of a clump, E1 = { j : p_j <= p1 } may be its index marker (p1 <= p2, so E1 is a subset of E2;
// a NaN p fails both comparisons and is in neither).  The order is ascending p, equal p by ascending marker index: a stable sort of the
// markers of E2 on p.  Because p1 <= p2 the markers of E1 are the first n_e1 of that order, so ONE rank array serves both sets:
// rank[j] = -1 outside E2, else the place of j in the order, and j is in E1 iff 0 <= rank[j] < n_e1.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace gvc {

struct Plan {
    std::vector<int> rank;      // M: the place of marker j in the order of E2, -1 outside E2
    std::vector<int> order;     // n_e2: the markers of E2 in that order; the first n_e1 of them are E1
    int64_t n_e1 = 0, n_e2 = 0;
    std::vector<int> pairs;     // the launch list: (I, J) of every block that holds an in-band pair and a marker of E2 in both row groups
    int64_t blocks_in_band = 0; // the blocks that hold an in-band pair (section 19's list), filtered or not
    double pairs_e2 = 0.0;      // the ordered in-band pairs (j, k) with both markers in E2, self included
};

// hi: the last in-band index of every marker (gvw::Window::hi), dmax: the most row groups a row group reaches ahead.  O(M log M).
inline Plan make_plan(const double* p, double p1, double p2, const int64_t* hi, int64_t dmax, int64_t M) {
    Plan pl;
    pl.rank.assign((size_t)M, -1);
    for (int64_t j = 0; j < M; j++)
        if (p[j] <= p2) pl.order.push_back((int)j);
    std::stable_sort(pl.order.begin(), pl.order.end(), [p](int a, int b) { return p[a] < p[b]; });
    pl.n_e2 = (int64_t)pl.order.size();
    for (int64_t q = 0; q < pl.n_e2; q++) {
        pl.rank[(size_t)pl.order[(size_t)q]] = (int)q;
        if (p[pl.order[(size_t)q]] <= p1) pl.n_e1 = q + 1;
    }
    // cnt[j]: the markers of E2 below j
    std::vector<int64_t> cnt((size_t)M + 1, 0);
    for (int64_t j = 0; j < M; j++) cnt[(size_t)j + 1] = cnt[(size_t)j] + (pl.rank[(size_t)j] >= 0);
    int64_t over = 0;
    for (int64_t j = 0; j < M; j++)
        if (pl.rank[(size_t)j] >= 0) over += cnt[(size_t)hi[j] + 1] - cnt[(size_t)j + 1];
    pl.pairs_e2 = (double)pl.n_e2 + 2.0 * (double)over;
    // the blocks (I, I + d) with d outermost, the order of section 19's list
    const int64_t nrg = (M + 63) / 64;
    auto reach = [&](int64_t I) { return hi[std::min(I * 64 + 63, M - 1)] / 64 - I; };
    auto holds = [&](int64_t I) { return cnt[(size_t)std::min(I * 64 + 64, M)] > cnt[(size_t)(I * 64)]; };
    for (int64_t d = 0; d <= dmax; d++)
        for (int64_t I = 0; I + d < nrg; I++)
            if (reach(I) >= d) {
                pl.blocks_in_band++;
                if (holds(I) && holds(I + d)) {
                    pl.pairs.push_back((int)I);
                    pl.pairs.push_back((int)(I + d));
                }
            }
    return pl;
}

}  // namespace gvc
