// gv_tune.hip -- the work decompositions of the streaming kernels: the candidates of a shard (plan_decomps), the pick among them
// by measurement on the resident data (autotune_ks), and the picks persisted in the cache file and shipped in gv_tune_builtin.h.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include "gv_internal.h"
#include "gv_tune_builtin.h"

namespace gvi {

// ---- persisted picks ---------------------------------------------------------------------------------------------
// The decomposition picked for a (device ISA, CU count, N, M, layout) is appended to a small text file under $GV_TUNE_CACHE_DIR, else
// $XDG_CACHE_HOME/gvamp_amd, else ~/.cache/gvamp_amd (GV_TUNE_CACHE=0: neither read nor written), so that only the first
// run on a shape pays for the measurement.  One line per key, the last matching line wins; a line is written with one
// O_APPEND write (ranks of a sharded job may share the file).  Results never depend on the pick (exact integer
// accumulation), so a stale or foreign line can cost time, never correctness; every loaded pick is range-checked.
constexpr int GV_TUNE_VERSION = 9;   // bump when the candidate set or the line format changes shape (9: tail hybrids, ticket-dealt items)
#ifndef GV_KERNEL_SRC_HASH
#error "build with -DGV_KERNEL_SRC_HASH=\"...\" (gvamp_amd/build.py computes it from the streaming-kernel sources)"
#endif
static std::string tune_cache_file() {
    const char* on = getenv("GV_TUNE_CACHE");
    if (on && atoi(on) == 0) return std::string();
    std::string dir;
    if (const char* d = getenv("GV_TUNE_CACHE_DIR")) dir = d;
    else if (const char* x = getenv("XDG_CACHE_HOME")) dir = std::string(x) + "/gvamp_amd";
    else if (const char* h = getenv("HOME")) dir = std::string(h) + "/.cache/gvamp_amd";
    else return std::string();
    return dir + "/decomp.txt";
}
static std::string tune_key(gv_ctx* c) {
    hipDeviceProp_t pr;
    if (hipGetDeviceProperties(&pr, c->device) != hipSuccess) { (void)hipGetLastError(); return std::string(); }
    // the device is identified by ISA target and CU count (the marketing name is not stable: it reads empty under rocprofv3)
    char buf[256];
    // GV_KERNEL_SRC_HASH (gvamp_amd/build.py: sha256 of gv_mfma.hip + gv_mfma.h) ties a line to the kernels it was measured on: a
    // pick made for other kernel sources is never read back
    // (D: work items dealt by ticket or taken by block index -- picks measured under one mapping are not read back under the other)
    snprintf(buf, sizeof(buf), "v%d|%s|%s|%d|%lld|%lld|L%d|D%d|", GV_TUNE_VERSION, GV_KERNEL_SRC_HASH, pr.gcnArchName,
             pr.multiProcessorCount, (long long)c->N, (long long)c->M, c->plan.layout, c->deal.ctr ? 1 : 0);
    return buf;
}
// markers per K-block of the Ax side: 256 on the stripe layout, 64 on the tile layout (which the Ax side walks transposed)
static inline int64_t ax_kb_markers(const gvm::Plan& pl) { return pl.layout == 1 ? 64 : 256; }
// does no int32 digit sum of an Ax-side pass under d wrap, whatever the vector?  (gvm::ax_bound_ok, gv_mfma.h)
static bool ax_bound_ok(const gv_ctx* c, const gvm::Decomp& d) {
    return gvm::ax_bound_ok(d, c->plan.nkb_n, ax_kb_markers(c->plan), c->M);
}
// is decomposition d admissible for side (0: ATx / stripes_m, 1: Ax / stripes_n) of this context?  why (may be NULL): set to 1 when
// the int32 bound of the Ax side is what refuses it
static bool decomp_ok(const gv_ctx* c, const gvm::Decomp& d, int side, int* why = nullptr) {
    const gvm::Plan& pl = c->plan;
    const int64_t nkb = side ? pl.nkb_n : pl.nkb_m, nrg = side ? pl.nrg_n : pl.nrg_m;
    // (a fast necessary condition: fewer than min_ks segments cannot keep the bound; whether d's own segments do is asked below)
    const int64_t min_ks = side ? (c->M * gvm::GV_AX_ENTRY_MAX + gvm::GV_I32_MAX - 1) / gvm::GV_I32_MAX : 1;
    if (why) *why = 0;
    int64_t pieces;
    if (d.skL > 0) {
        if (side && min_ks > 1 && d.skL >= 8) { if (why) *why = 1; return false; }     // balanced ranges and whole quads: never past one segment's worth
        if (d.skL < 8 || nkb < 2 || d.piv < 0 || d.piv > (nrg + 3) / 4) return false;
        pieces = (nkb + d.skL - 1) / d.skL + 1;
    } else {
        if (d.ks < 1 || d.ks > 64 || d.ks > nkb || d.piv != 0) return false;
        if (d.ks < min_ks) { if (why) *why = 1; return false; }
        pieces = d.ks;
    }
    if (!(d.taper >= 0.f && d.taper < 1.f) || !(d.geo >= 0.f && d.geo < 1.f) || (d.geo > 0.f && d.skL > 0) || (d.prio != 0 && d.prio != 1)) return false;
    if (d.occ != 0 && d.occ != 2 && d.occ != 3) return false;
    if (!(d.xskew >= -0.2f && d.xskew <= 0.2f) || (d.xskew != 0.f && d.skL > 0)) return false;
    if (side && !ax_bound_ok(c, d)) { if (why) *why = 1; return false; }
    return (size_t)pieces * 4 * nrg * (side ? pl.rows_n : 64) * 8 * 4 <= pl.partial_bytes;
}
static bool tune_cache_load(gv_ctx* c) {
    const std::string path = tune_cache_file(), key = tune_key(c);
    if (path.empty() || key.empty()) return false;
    FILE* f = fopen(path.c_str(), "r");
    if (!f) return false;
    char line[1024];
    gvm::Decomp got[4];
    bool have = false;
    while (fgets(line, sizeof(line), f)) {
        if (strncmp(line, key.c_str(), key.size()) != 0) continue;
        gvm::Decomp d[4];
        long long sk[4], pv[4];
        {
            const char* q = line + key.size();
            int nread = 0, ok = 1;
            for (int k = 0; k < 4 && ok; k++) {
                if (sscanf(q, "%d %lld %lld %d %f %f %d %f%n", &d[k].ks, &sk[k], &pv[k], &d[k].prio, &d[k].taper, &d[k].geo, &d[k].occ, &d[k].xskew,
                           &nread) != 8)
                    ok = 0;
                q += nread;
            }
            if (!ok) continue;
        }
        for (int k = 0; k < 4; k++) { d[k].skL = sk[k]; d[k].piv = pv[k]; got[k] = d[k]; }
        have = true;
    }
    fclose(f);
    if (!have) return false;
    for (int k = 0; k < 4; k++)
        if (!decomp_ok(c, got[k], k >> 1)) return false;
    if (!c->ks_fixed_m) { c->plan.dm[0] = got[0]; c->plan.dm[1] = got[1]; }
    if (!c->ks_fixed_n) { c->plan.dn[0] = got[2]; c->plan.dn[1] = got[3]; }
    return true;
}
// picks shipped in-tree for this very build of the kernels (gv_tune_builtin.h); GV_TUNE_BUILTIN=0 ignores them
static bool tune_builtin_load(gv_ctx* c) {
    const char* on = getenv("GV_TUNE_BUILTIN");
    if ((on && atoi(on) == 0) || strcmp(GV_BUILTIN_FOR_HASH, GV_KERNEL_SRC_HASH) != 0) return false;
    hipDeviceProp_t pr;
    if (hipGetDeviceProperties(&pr, c->device) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (strncmp(pr.gcnArchName, "gfx950", 6) != 0 || pr.multiProcessorCount != 256) return false;
    for (const BuiltinPick& b : GV_BUILTIN_PICKS) {
        if (b.N != c->N || b.M != c->M || b.layout != c->plan.layout || b.N == 0) continue;
        for (int k = 0; k < 4; k++)
            if (!decomp_ok(c, b.d[k], k >> 1)) return false;
        if (!c->ks_fixed_m) { c->plan.dm[0] = b.d[0]; c->plan.dm[1] = b.d[1]; }
        if (!c->ks_fixed_n) { c->plan.dn[0] = b.d[2]; c->plan.dn[1] = b.d[3]; }
        return true;
    }
    return false;
}
static void tune_cache_store(gv_ctx* c) {
    const std::string path = tune_cache_file(), key = tune_key(c);
    if (path.empty() || key.empty() || c->ks_fixed_m || c->ks_fixed_n) return;   // overrides are not picks
    const size_t slash = path.rfind('/');
    std::string dir = path.substr(0, slash);
    for (size_t i = 1; i <= dir.size(); i++)                                      // mkdir -p
        if (i == dir.size() || dir[i] == '/') (void)mkdir(dir.substr(0, i).c_str(), 0755);
    const gvm::Decomp* d[4] = {&c->plan.dm[0], &c->plan.dm[1], &c->plan.dn[0], &c->plan.dn[1]};
    char buf[1024];
    int n = snprintf(buf, sizeof(buf), "%s", key.c_str());
    // xskew is written as 0: which four XCDs are ahead changes with the box and the allocation (profiles/r6_xcd_skew.txt), so a cached
    // sign could pin the losing skew for every later process that shares the file
    for (int k = 0; k < 4; k++)
        n += snprintf(buf + n, sizeof(buf) - n, "%d %lld %lld %d %.2f %.2f %d %.3f ", d[k]->ks, (long long)d[k]->skL, (long long)d[k]->piv, d[k]->prio,
                      d[k]->taper, d[k]->geo, d[k]->occ, 0.0);
    n += snprintf(buf + n, sizeof(buf) - n, "\n");
    const int fd = open(path.c_str(), O_WRONLY | O_APPEND | O_CREAT, 0644);
    if (fd < 0) return;
    ssize_t w = write(fd, buf, (size_t)n);
    (void)w;
    close(fd);
}

// The work decomposition of each streaming-kernel class (ATx, two-vector ATx, Ax, two-vector Ax) is picked by measurement
// among the candidates gv_set_dims lists, once per shard, before its first matvec in kernel mode 1, on the resident stripes
// with throw-away vectors (no counters, no collectives) -- unless an earlier run on the same (device, N, M) left its picks in
// the cache above.  Protocol, sized so that the cold cost stays a fraction of a second at 100 GB:
//   stage A  the uniform splits short-listed by the cost model and the balanced grids, without / with their natural priority
//            setting;  stage B  on the winner only: progress-based wave priority (uniform splits), then tapered segment
//            lengths 0.5 / 0.9 (uniform splits with more than one segment), then longer segments for one set of four XCDs (both
//            signs), then two workgroups per CU instead of three.  At most ~20 timed candidates per class.
//   long kernels (>= 4 ms): ONE run of the product being tuned per candidate -- at that length neither the clocks nor what
//            ran before move the result; short kernels: one untimed pair, then two batches of products of the side being tuned,
//            each timed on its own inside the alternating Ax -> ATx sequence the solvers issue (the other side on its current
//            pick, untimed) -- a decomposition that won by 2 % back to back with itself was measured 10 % behind inside the
//            alternating sequence (N = 50k x M = 200k, two-vector Ax); the faster batch counts (one launch in 20-30 of some
//            decompositions lands 15-35 % above the rest).  Operands are pseudo-random: a constant vector populates one digit
//            plane and ranks the candidates differently.
// Results do not depend on the decomposition (exact integer accumulation), so tuning never changes a bit of output.
int autotune_ks(gv_ctx* c) {
    c->ks_tuned = true;
    c->tune_seconds = 0.0;
    c->tune_source = 0;
    if ((c->ks_fixed_m && c->ks_fixed_n) || !c->have_stripes || c->M <= 0 || !c->have_stats) { c->tune_source = 3; return 0; }
    if (tune_cache_load(c)) { c->tune_source = 2; return 0; }
    if (tune_builtin_load(c)) { c->tune_source = 4; return 0; }
    const auto wall0 = std::chrono::steady_clock::now();
    gvm::Plan& pl = c->plan;
    double *xm = nullptr, *wm = nullptr, *wm2 = nullptr, *pn = nullptr, *zn = nullptr, *zn2 = nullptr;
    auto done = [&](int rc) {
        for (double* q : {xm, wm, wm2, pn, zn, zn2}) if (q) (void)hipFree(q);
        pl.ev0 = pl.ev1 = nullptr;
        c->tune_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - wall0).count();
        return rc;
    };
    if (hipMalloc(&xm, sizeof(double) * c->M) != hipSuccess || hipMalloc(&wm, sizeof(double) * c->M) != hipSuccess ||
        hipMalloc(&wm2, sizeof(double) * c->M) != hipSuccess || hipMalloc(&pn, sizeof(double) * c->npad) != hipSuccess ||
        hipMalloc(&zn, sizeof(double) * c->npad) != hipSuccess || hipMalloc(&zn2, sizeof(double) * c->npad) != hipSuccess) {
        (void)hipGetLastError();
        return done(0);                      // no room for the scratch vectors: keep the model's pick
    }
    gvk::fill_hash(c->stream, xm, c->M, 1);           // representative operands: every digit plane populated
    gvk::fill_hash(c->stream, pn, c->npad, 2);
    pl.ev0 = pl.ev1 = nullptr;
    constexpr int TUNE_MAXREPS = 12;
    hipEvent_t tev[2 * TUNE_MAXREPS] = {};
    for (hipEvent_t& e : tev)
        if (hipEventCreate(&e) != hipSuccess) { (void)hipGetLastError(); e = nullptr; }
    struct EvGuard { hipEvent_t* e; int n; ~EvGuard() { for (int i = 0; i < n; i++) if (e[i]) (void)hipEventDestroy(e[i]); } } ev_guard{tev, 2 * TUNE_MAXREPS};
    // side: 0 = both products (the pair the solvers issue), 1 = Ax side only, 2 = ATx side only
    auto run = [&](int dual, int side) {
        if (side != 2) {
            if (dual) gvm::ax2(c->stream, pl, xm, xm, c->mave, c->msig, c->mask2, c->npad, 1.0, c->red_partial, zn, zn2);
            else gvm::ax(c->stream, pl, xm, c->mave, c->msig, c->mask2, c->npad, 1.0, c->red_partial, zn);
        }
        if (side != 1) {
            if (dual) gvm::atx2(c->stream, pl, pn, pn, c->npad, c->mave, c->msig, 1.0, c->red_partial, wm, wm2, nullptr, nullptr, 1.0, 0.0);
            else gvm::atx(c->stream, pl, pn, c->npad, c->mave, c->msig, 1.0, c->red_partial, wm);
        }
    };
    auto timed = [&](int dual, int side, int reps) -> double {   // ms per repetition
        (void)hipEventRecord(c->ev0, c->stream);
        for (int r = 0; r < reps; r++) run(dual, side);
        (void)hipEventRecord(c->ev1, c->stream);
        if (hipEventSynchronize(c->ev1) != hipSuccess) return -1.0;
        float ms = 0;
        (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
        return ms / reps;
    };
    // short kernels: the product being tuned alone, timed launch by launch INSIDE the alternating sequence the solvers issue (the
    // other side runs, untimed, before every timed product): ms per product, prepare / quantise / finalise included.  Timing the
    // pair diluted a 5 % difference on one side to 2.5 % of a number that moves by 1-2 % from batch to batch.
    auto timed_side = [&](int dual, bool ax_side, int reps) -> double {
        if (reps > TUNE_MAXREPS) reps = TUNE_MAXREPS;
        for (int r = 0; r < reps; r++) {
            if (!tev[2 * r] || !tev[2 * r + 1]) return -1.0;
            run(dual, ax_side ? 2 : 1);
            (void)hipEventRecord(tev[2 * r], c->stream);
            run(dual, ax_side ? 1 : 2);
            (void)hipEventRecord(tev[2 * r + 1], c->stream);
        }
        if (hipEventSynchronize(tev[2 * reps - 1]) != hipSuccess) return -1.0;
        double tot = 0.0;
        for (int r = 0; r < reps; r++) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, tev[2 * r], tev[2 * r + 1]);
            tot += ms;
        }
        return tot / reps;
    };
    const bool verbose = getenv("GV_AUTOTUNE_VERBOSE") != nullptr;
    if (timed(0, 0, 1) < 0) { KCHK(c); return done(1); }        // clocks and caches up before anything is compared
    for (int step = 0; step < 4; step++) {
        const int dual = step >> 1;
        const bool is_ax = (step & 1) == 0;             // Ax side first, then the ATx side against the tuned Ax
        const int cls = is_ax ? 2 + dual : dual;        // 0 ATx, 1 two-vector ATx, 2 Ax, 3 two-vector Ax
        if (is_ax ? c->ks_fixed_n : c->ks_fixed_m) continue;
        const std::vector<gvm::Decomp>& cand = is_ax ? c->dec_cand_n : c->dec_cand_m;
        gvm::Decomp& d = is_ax ? pl.dn[dual] : pl.dm[dual];
        if (cand.empty()) continue;
        d = cand[0];
        const double t_pair = timed(dual, 0, 1);        // sizes the protocol of this class (and warms it)
        if (t_pair < 0) { KCHK(c); return done(1); }
        const bool solo = t_pair >= 8.0;                // both products >= ~4 ms
        const int side = solo ? (is_ax ? 1 : 2) : 0;
        int reps = solo ? 1 : (int)(8.0 / (t_pair > 1e-3 ? t_pair : 1e-3)) + 1;     // (timed products per batch; the other side runs beside each)
        if (reps > 8) reps = 8;
        auto measure = [&](const gvm::Decomp& cd) -> double {
            d = cd;
            if (!solo && timed(dual, 0, 1) < 0) return -1.0;   // untimed: the first launch of a new grid shape
            // short kernels: two batches, the faster one counts.  One launch in 20-30 of some decompositions lands 15-35 % above
            // the rest (profiles/r6_launch_dist_shard.txt); a single batch of 2-8 pairs that catches one ranks its candidate by
            // the accident -- round 5's table held a pick 2.5 % behind its own priority variant that way.
            double t = solo ? timed(dual, side, reps) : timed_side(dual, is_ax, reps);
            if (!solo && t >= 0) {
                const double t2 = timed_side(dual, is_ax, reps);
                if (t2 < 0) return -1.0;
                if (t2 < t) t = t2;
            }
            if (verbose)
                fprintf(stderr, "[gvamp autotune] class %d ks %d skL %lld whole quads %lld prio %d taper %.1f geo %.2f occ %d xskew %.3f : %.4f ms / %s\n", cls, cd.ks,
                        (long long)cd.skL, (long long)cd.piv, cd.prio, cd.taper, cd.geo, cd.occ, cd.xskew, t, "product");
            return t;
        };
        gvm::Decomp best = cand[0];
        double best_t = -1;
        auto consider = [&](const gvm::Decomp& cd) -> int {
            if (is_ax && !ax_bound_ok(c, cd)) return 0;      // a taper or skew of the winner may stretch a segment past the int32 bound
            const double t = measure(cd);
            if (t < 0) return 1;
            if (best_t < 0 || t < best_t * 0.997) { best_t = t; best = cd; }   // the list order breaks near-ties
            return 0;
        };
        // stage A: uniform splits without priority, balanced grids (which carry their priority setting)
        bool any_plain = false;
        for (const gvm::Decomp& cd : cand) any_plain |= cd.skL <= 0 && cd.prio == 0;
        for (const gvm::Decomp& cd : cand) {
            if (cd.skL <= 0 && cd.prio != 0 && cd.geo == 0.f && any_plain) continue;
            if (consider(cd)) { d = cand[0]; KCHK(c); return done(1); }
        }
        // stage B on the winner: priority, then taper
        if (best.skL <= 0) {
            bool prio_listed = false;
            for (const gvm::Decomp& cd : cand) prio_listed |= cd.skL <= 0 && cd.prio == 1 && cd.ks == best.ks;
            if (best.prio == 0 && prio_listed) {
                gvm::Decomp t = best; t.prio = 1;
                if (consider(t)) { d = cand[0]; KCHK(c); return done(1); }
            }
            if (best.ks > 1 && best.taper == 0.f && best.geo == 0.f) {      // (a geometric split has its own segment lengths)
                const gvm::Decomp base = best;
                for (float tp : {0.5f, 0.9f}) {
                    gvm::Decomp t = base; t.taper = tp;
                    if (consider(t)) { d = cand[0]; KCHK(c); return done(1); }
                }
            }
        }
        // ... then more work for four of the eight XCDs (Decomp::xskew), on a winner whose quads have at least two segments.  WHICH four
        // finish equal shares first belongs to the box and to where the allocation landed (profiles/r6_xcd_skew.txt): both signs are
        // measured on the resident data, and the better one is pushed once more if it beat the equal shares
        // (block-index mapping only: dealt launches ignore xskew -- an XCD that is ahead draws more items by itself)
        if (best.skL <= 0 && best.ks >= 2 && !pl.deal) {
            const gvm::Decomp base = best;
            const double t_base = best_t;
            for (float sk : {0.02f, -0.02f}) {
                gvm::Decomp t = base; t.xskew = sk;
                if (consider(t)) { d = cand[0]; KCHK(c); return done(1); }
            }
            if (best.xskew != 0.f && best_t < t_base) {
                gvm::Decomp t = best; t.xskew = best.xskew > 0.f ? 0.035f : -0.035f;
                if (consider(t)) { d = cand[0]; KCHK(c); return done(1); }
            }
        }
        // ... then two workgroups per CU instead of three, on the winner and on the best geometric split (which is what gains from it
        // where anything does: many short workgroups late in the launch)
        {
            const gvm::Decomp base = best;
            gvm::Decomp t = base; t.occ = 2;
            if (consider(t)) { d = cand[0]; KCHK(c); return done(1); }
            for (const gvm::Decomp& cd : cand)
                if (cd.geo > 0.f && cd.ks >= 6 && !(cd.ks == base.ks && cd.geo == base.geo)) {
                    gvm::Decomp g = cd; g.occ = 2;
                    if (consider(g)) { d = cand[0]; KCHK(c); return done(1); }
                    break;
                }
        }
        d = best;
        if (verbose)
            fprintf(stderr, "[gvamp autotune] class %d -> ks %d skL %lld whole quads %lld prio %d taper %.1f geo %.2f occ %d xskew %.3f\n", cls, d.ks,
                    (long long)d.skL, (long long)d.piv, d.prio, d.taper, d.geo, d.occ, d.xskew);
    }
    KCHK(c);
    c->tune_source = 1;
    tune_cache_store(c);
    return done(0);
}

// Geometry of the streaming kernels for the layout that will be built (c->want_tile) and the candidate work decompositions
// of each side.  Called by gv_set_dims and again by ingest when gv_set_layout changed the layout in between.
int plan_decomps(gv_ctx* c) {
    const int64_t N = c->N, M = c->M;
    gvm::Plan& pl = c->plan;
    pl.M = M; pl.N = N;
    pl.deal = c->deal.ctr ? &c->deal : nullptr;
    pl.nrg_m = (M + 63) / 64;  pl.nkb_m = (N + 255) / 256;
    pl.nrg_n = (N + 63) / 64;  pl.nkb_n = (M + 255) / 256;
    pl.layout = c->want_tile ? 1 : 0;
    pl.rows_n = 64;
    if (c->want_tile) {   // one layout: the Ax side walks the marker-group-major super-blocks transposed
        pl.nrg_n = pl.nkb_m;       // row groups of 256 individuals
        pl.nkb_n = pl.nrg_m;       // K-steps of 64 markers
        pl.rows_n = 256;
    }
    // K-splits.  A launch is W = ceil(nrg / 4) * ks workgroups, each walking nkb / ks K-blocks; 768 are resident at a time
    // (256 CUs x 3).  Sweeps on MI355X (GV_KS_M / GV_KS_N overrides; N = 50k ... 400k, M = 125k ... 1M) show 2-7 % between
    // neighbouring splits, from three effects no closed form ranks reliably: a short last round of workgroups running at
    // their own ceiling (a workgroup keeps 32 KiB in flight, ~450 of them saturate HBM), stragglers of the last round
    // against an emptying chip, and per-workgroup prologue / epilogue / partial sums (~40 K-blocks' worth).  So a small
    // cost model only SHORT-LISTS three candidates here
    //   per = nkb/ks + 40 ;  W <= 768: T = per * max(W, 448) / 768 ;  W > 768: T = per * W / 768 + straggle * per
    // and the pick among them is MEASURED once per shard on the resident data (autotune_ks, before the first matvec).
    // Results do not depend on the split (exact integer accumulation), so tuning never changes a bit of output.
    auto rank_ks = [](int64_t nrg, int64_t nkb, int64_t min_ks, double straggle, int* out3) {
        const int64_t nq = (nrg + 3) / 4;
        out3[0] = out3[1] = out3[2] = (int)(min_ks > 1 ? min_ks : 1);
        if (nq <= 0 || nkb <= 0) return;
        int64_t hi = nkb / 32 > 1 ? nkb / 32 : 1;                  // never fewer than 32 K-blocks per workgroup
        if (hi > 64) hi = 64;
        if (min_ks > hi) hi = min_ks;
        double cost[3] = {0, 0, 0};
        int n = 0;
        for (int64_t ks = min_ks > 1 ? min_ks : 1; ks <= hi && ks <= nkb; ks++) {
            const double per = (double)nkb / (double)ks + 40.0;
            const int64_t W = nq * ks;
            const double t = W <= 768 ? per * (double)(W > 448 ? W : 448) / 768.0 : per * (double)W / 768.0 + straggle * per;
            int pos = n < 3 ? n : 3;                                // insertion into the three cheapest
            while (pos > 0 && t < cost[pos - 1]) pos--;
            if (pos >= 3) continue;
            for (int j = (n < 3 ? n : 2); j > pos; j--) { cost[j] = cost[j - 1]; out3[j] = out3[j - 1]; }
            cost[pos] = t;
            out3[pos] = (int)ks;
            if (n < 3) n++;
        }
        for (int j = n; j < 3; j++) out3[j] = out3[n > 0 ? n - 1 : 0];
    };
    // Ax side: the int32 bound (gv_mfma.h, ax_bound_ok).  min_ks_n: the fewest EQUAL segments that keep it; every candidate below is
    // asked with its own segment lengths (ax_ok).  gv_set_dims has refused a shard that no split of 64 segments can serve.
    const int64_t kbm_n = ax_kb_markers(pl);
    int64_t min_ks_n = gvm::ax_min_ks(pl.nkb_n, kbm_n, M);
    if (min_ks_n < 1) min_ks_n = 1;
    auto ax_ok = [&](const gvm::Decomp& d) { return gvm::ax_bound_ok(d, pl.nkb_n, kbm_n, M); };
    int ks3_m[3], ks3_n[3];
    rank_ks(pl.nrg_m, pl.nkb_m, 1, 0.4, ks3_m);
    rank_ks(pl.nrg_n, pl.nkb_n, min_ks_n, 0.8, ks3_n);
    // balanced decomposition (k_mfma_matvec<., true>): cells per workgroup for a grid of G workgroups.  A segment is at most
    // min(skL, nkb) K-blocks long; on the Ax side it must respect the int32 bound that min_ks_n expresses.
    auto skL_of = [](int64_t nrg, int64_t nkb, int64_t G) -> int64_t {
        const int64_t U = ((nrg + 3) / 4) * nkb;
        if (U <= 0 || G <= 0) return 0;
        const int64_t L = (U + G - 1) / G;
        return L < 8 ? 8 : L;
    };
    // Candidate list per side, default first: the uniform splits in the model's order without priority, the same with
    // priority, then balanced grids of one and two workgroups per slot (always with priority: without it the staggered
    // workgroups of a balanced launch lose ~10 % to the arbiter's oldest-first tail).
    int prio_only = -1;                                    // GV_PRIO=0/1 (development): restrict to one setting
    if (const char* e = getenv("GV_PRIO")) prio_only = atoi(e) ? 1 : 0;
    // piv quads whole (0: as many whole rounds of 768 as the quads allow), the rest balanced over G workgroups; the pieces a row
    // of the remainder is cut into are bounded so that the int32 partial sums stay below 1 GB (4 planes x 32 B per row and piece)
    auto hybrid_of = [](int64_t nrg, int64_t nkb, int64_t rows, int64_t piv, int64_t G, double max_bytes = 1.0e9) -> gvm::Decomp {
        gvm::Decomp h;
        const int64_t nq = (nrg + 3) / 4;
        if (piv <= 0) piv = nq / 768 * 768;
        if (piv <= 0 || piv >= nq || nkb < 2 || G <= 0) return h;
        const int64_t cells = (nq - piv) * nkb;
        int64_t maxp = (int64_t)(max_bytes / (128.0 * (double)nrg * (double)rows));
        if (maxp > 60) maxp = 60;
        if (maxp < 3) return h;
        int64_t L = (cells + G - 1) / G;
        const int64_t Lmin = (nkb + maxp - 2) / (maxp - 1);
        if (L < Lmin) L = Lmin;
        if (L < 8) L = 8;
        h.ks = 1; h.skL = L; h.piv = piv; h.prio = 1;
        return h;
    };
    const bool dealt = c->deal.ctr != nullptr;      // work items dealt by ticket (gv_create)
    // (geo_side: the Ax side -- the many-segment geometric splits are listed there, and every uniform split is asked for the int32 bound)
    auto build = [&](const int* ks3, int64_t nrg, int64_t nkb, int64_t rows, bool balanced_ok, int64_t min_ks_u, bool geo_side, std::vector<gvm::Decomp>& out) {
        out.clear();
        for (int prio = 0; prio < 2; prio++) {
            if (prio_only >= 0 && prio != prio_only) continue;
            for (int j = 0; j < 3; j++) {
                if (j > 0 && (ks3[j] == ks3[0] || (j == 2 && ks3[2] == ks3[1]))) continue;
                gvm::Decomp d; d.ks = ks3[j]; d.skL = 0; d.prio = prio;
                if (geo_side && !ax_ok(d)) continue;
                out.push_back(d);
            }
        }
        // geometric splits (big first): ks segments per quad, segment j = geo^j of segment 0, every one at least 8 K-blocks long.
        // Many short segments (6-8): Ax side only -- measured in-process against the tuner's picks
        // (profiles/r4_decomp_ab_inprocess.txt) they gain 1-2.4 % on the Ax classes of 12.5 GB and 2.5 GB shards and lose 1-10 % on
        // every ATx class (GV_TUNE_GEO=1 lists them there too).  Two to four segments: both sides.  A launch of nq < 768 whole-K
        // workgroups (one round that does not fill the chip) streams with nq of the 768 slots for its
        // whole length and ends on the spread of their speeds; a short second segment fills the idle slots for the first part of
        // the launch instead: two-vector ATx of the 8-GPU shard (N = 400k x M = 125k, 489 quads, tile layout), per-launch
        // distributions of 80 launches each in one process (profiles/r6_launch_dist_shard.txt): ks 1 p50 2.016 ms with 3 launches
        // of 80 at 2.2-2.7 ms, ks 2 geo 0.5 p50 1.904 ms, max 1.941.  Just above a round (config 5's two-vector ATx, 782 quads): ks 4
        // geo 0.5 0.424 ms with no launch above 0.431 against the hybrid's 0.441 with 4 of 30 at 0.49-0.56.
        if (prio_only != 0) {
            std::vector<std::pair<int, float>> gks;
            for (const auto& gk : {std::pair<int, float>{2, 0.5f}, {2, 0.35f}, {3, 0.5f}, {4, 0.5f}}) gks.push_back(gk);
            if (geo_side || getenv("GV_TUNE_GEO")) for (const auto& gk : {std::pair<int, float>{6, 0.6f}, {8, 0.65f}, {8, 0.8f}}) gks.push_back(gk);
            for (const auto& gk : gks) {
                double tot = 0.0, wlast = 1.0;
                for (int j = 0; j < gk.first; j++) { tot += wlast; if (j + 1 < gk.first) wlast *= gk.second; }
                if ((double)nkb * wlast / tot < 8.0 || gk.first < min_ks_u) continue;
                bool dup = false;
                for (const gvm::Decomp& o : out) dup |= o.skL <= 0 && o.ks == gk.first && o.geo == gk.second;
                if (dup) continue;
                gvm::Decomp d; d.ks = gk.first; d.skL = 0; d.prio = 1; d.geo = gk.second;
                if (geo_side && !ax_ok(d)) continue;
                out.push_back(d);
            }
        }
        if (balanced_ok && prio_only != 0 && nkb >= 2) {
            // hybrid: whole rounds of the 768 resident workgroups go one quad per workgroup (in step over K), the quads that are
            // left over are cut into 768 balanced ranges -- for quad counts just above a multiple of 768 (gv_mfma.hip).  Listed
            // before the fully balanced grids: on a tie it is the one that fetches every digit block once per XCD
            gvm::Decomp h = hybrid_of(nrg, nkb, rows, 0, 768);
            if (h.skL > 0) out.push_back(h);
            for (int r = 1; r <= 2; r++) {
                gvm::Decomp d; d.ks = 1; d.skL = skL_of(nrg, nkb, 768 * r); d.prio = 1;
                if (d.skL > 0) out.push_back(d);
            }
            // dealt launches: hybrids whose remainder is a real TAIL -- the last 7 % / 10 % of the quads in ranges of ~80 / ~160 cells
            // (16 KiB per cell, ~9 GB/s per resident workgroup: 150 / 300 us; never shorter than the partial sums allow: up to 2 GB
            // here).  The whole quads are drawn first; an XCD that frees its slots early draws tail ranges instead of idling.  Only
            // where the whole quads fill the chip at least once.
            if (dealt && (nrg + 3) / 4 >= 768) {
                const int64_t nq = (nrg + 3) / 4;
                for (const auto& tl : {std::pair<double, int64_t>{0.07, 80}, {0.10, 160}}) {
                    int64_t tq = (int64_t)(tl.first * (double)nq + 0.5);
                    if (tq < 1) tq = 1;
                    const int64_t G = (tq * nkb + tl.second - 1) / tl.second;
                    gvm::Decomp t = hybrid_of(nrg, nkb, rows, nq - tq, G, 2.0e9);
                    bool dup = t.skL <= 0 || t.skL > nkb;
                    for (const gvm::Decomp& o : out) dup |= o.skL == t.skL && o.piv == t.piv;
                    if (!dup) out.push_back(t);
                }
            }
        }
        // dealt launches, Ax side: a few long segments followed by a longer geometric tail (the last of 12 segments is ~1 / 50 of the first)
        if (dealt && geo_side && prio_only != 0 && 12 >= min_ks_u) {
            double tot = 0.0, wlast = 1.0;
            for (int j = 0; j < 12; j++) { tot += wlast; if (j + 1 < 12) wlast *= 0.7; }
            gvm::Decomp d; d.ks = 12; d.skL = 0; d.prio = 1; d.geo = 0.7f;
            if ((double)nkb * wlast / tot >= 8.0 && ax_ok(d)) out.push_back(d);
        }
    };
    build(ks3_m, pl.nrg_m, pl.nkb_m, 64, true, 1, false, c->dec_cand_m);
    build(ks3_n, pl.nrg_n, pl.nkb_n, pl.rows_n, min_ks_n <= 1, min_ks_n, true, c->dec_cand_n);
    c->ks_tuned = c->ks_fixed_m = c->ks_fixed_n = false;
    // overrides (development): GV_KS_M / GV_KS_N fix a uniform K-split of the ATx / Ax kernels, GV_SK_M / GV_SK_N a balanced
    // grid of that many workgroups (both with the priority setting of GV_PRIO, default off / on), GV_AUTOTUNE=0 keeps the
    // first candidate
    auto fix = [&](std::vector<gvm::Decomp>& cand, bool& fixed, gvm::Decomp d) { cand.assign(1, d); fixed = true; };
    const float taper_env = getenv("GV_TAPER") ? (float)atof(getenv("GV_TAPER")) : 0.f;
    const float geo_env = getenv("GV_GEO") ? (float)atof(getenv("GV_GEO")) : 0.f;
    if (const char* e = getenv("GV_KS_M")) {
        int v = atoi(e);
        if (v >= 1 && v <= pl.nkb_m && v <= 64) { gvm::Decomp d; d.ks = v; d.prio = prio_only == 1; d.taper = taper_env; d.geo = geo_env; fix(c->dec_cand_m, c->ks_fixed_m, d); }
    }
    if (const char* e = getenv("GV_KS_N")) {
        int v = atoi(e);
        gvm::Decomp d; d.ks = v; d.prio = prio_only == 1; d.taper = taper_env; d.geo = geo_env;
        if (v >= min_ks_n && v >= 1 && v <= pl.nkb_n && v <= 64 && ax_ok(d)) fix(c->dec_cand_n, c->ks_fixed_n, d);
    }
    if (const char* e = getenv("GV_SK_M")) {
        gvm::Decomp d; d.skL = skL_of(pl.nrg_m, pl.nkb_m, atoi(e)); d.prio = prio_only != 0;
        if (d.skL > 0) fix(c->dec_cand_m, c->ks_fixed_m, d);
    }
    if (const char* e = getenv("GV_SK_N")) {
        gvm::Decomp d; d.skL = min_ks_n > 1 ? 0 : skL_of(pl.nrg_n, pl.nkb_n, atoi(e)); d.prio = prio_only != 0;
        if (d.skL > 0) fix(c->dec_cand_n, c->ks_fixed_n, d);
    }
    // GV_HY_M / GV_HY_N = "<whole quads>:<workgroups of the remainder>": a hybrid decomposition (0 whole quads: whole rounds of 768)
    auto hy = [&](const char* e, int64_t nrg, int64_t nkb, int64_t rows) {
        long long piv = 0, G = 768;
        sscanf(e, "%lld:%lld", &piv, &G);
        gvm::Decomp d = hybrid_of(nrg, nkb, rows, piv, G);
        d.prio = prio_only != 0;
        return d;
    };
    if (const char* e = getenv("GV_HY_M")) {
        gvm::Decomp d = hy(e, pl.nrg_m, pl.nkb_m, 64);
        if (d.skL > 0) fix(c->dec_cand_m, c->ks_fixed_m, d);
    }
    if (const char* e = getenv("GV_HY_N")) {
        gvm::Decomp d = hy(e, pl.nrg_n, pl.nkb_n, pl.rows_n);
        if (d.skL > 0 && min_ks_n <= 1) fix(c->dec_cand_n, c->ks_fixed_n, d);
    }
    if (const char* e = getenv("GV_AUTOTUNE"))
        if (atoi(e) == 0) c->ks_fixed_m = c->ks_fixed_n = true;
    if (c->dec_cand_m.empty()) c->dec_cand_m.assign(1, gvm::Decomp());
    if (c->dec_cand_n.empty()) { gvm::Decomp d; d.ks = (int)(min_ks_n > 1 ? min_ks_n : 1); c->dec_cand_n.assign(1, d); }
    pl.dm[0] = pl.dm[1] = c->dec_cand_m[0];
    pl.dn[0] = pl.dn[1] = c->dec_cand_n[0];
    return 0;
}

}  // namespace gvi

using namespace gvi;

extern "C" {

int gv_tune_info(gv_ctx* c, double* seconds, int* source) {
    if (seconds) *seconds = c->tune_seconds;
    if (source) *source = c->ks_tuned ? c->tune_source : -1;
    return 0;
}
int gv_get_decomp(gv_ctx* c, gv_decomp_info* out4) {
    NEED(c, out4 != nullptr, "gv_get_decomp: out is NULL");
    const gvm::Decomp* d[4] = {&c->plan.dm[0], &c->plan.dm[1], &c->plan.dn[0], &c->plan.dn[1]};
    for (int k = 0; k < 4; k++) {
        out4[k].ks = d[k]->ks;
        out4[k].balanced_cells = d[k]->skL;
        out4[k].whole_quads = d[k]->skL > 0 ? d[k]->piv : 0;
        out4[k].prio = d[k]->prio;
        out4[k].taper = d[k]->taper;
        out4[k].geo = d[k]->geo;
        out4[k].wgs_per_cu = d[k]->occ == 2 ? 2 : 3;
        out4[k].xcd_skew = d[k]->xskew;
        out4[k].tuned = c->ks_tuned ? 1 : 0;
    }
    return 0;
}
int gv_set_decomp(gv_ctx* c, int cls, const gv_decomp_info* in) {
    REFUSE_DOSAGE(c, "gv_set_decomp", "no tunable decomposition (derived from N, M and the CU count)");
    NEED(c, !c->dense.resident, "gv_set_decomp: methylation data has no tunable decomposition (derived from N, M and the CU count)");
    NEED(c, cls >= 0 && cls <= 3 && in != nullptr, "gv_set_decomp: class 0..3 and a decomposition are required");
    NEED(c, c->have_stripes, "gv_set_decomp: no re-encoded layout resident yet (call it after the ingest)");
    gvm::Decomp d;
    d.ks = in->ks; d.skL = in->balanced_cells; d.piv = in->balanced_cells > 0 ? in->whole_quads : 0; d.prio = in->prio;
    d.taper = in->taper; d.geo = in->geo;
    NEED(c, in->wgs_per_cu == 0 || in->wgs_per_cu == 2 || in->wgs_per_cu == 3, "gv_set_decomp: wgs_per_cu is 0 (default), 2 or 3");
    d.occ = in->wgs_per_cu == 2 ? 2 : 0;
    d.xskew = in->balanced_cells > 0 ? 0.f : in->xcd_skew;
    if (d.skL > 0) d.ks = 1;
    int why = 0;
    const bool ok = decomp_ok(c, d, cls >> 1, &why);
    NEED(c, ok || why != 1, "gv_set_decomp: the decomposition is not admissible for this shard (int32 bound of the Ax side: the longest K-segment times 512 "
                           "must stay below 2^31)");
    NEED(c, ok, "gv_set_decomp: the decomposition is not admissible for this shard (range, or too many pieces for the partial-sum buffer)");
    (cls >> 1 ? c->plan.dn : c->plan.dm)[cls & 1] = d;
    return 0;
}

}  // extern "C"
