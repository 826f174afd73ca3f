// main_real.cpp -- real-data driver mirroring the reference's main_real.cpp:13-599.  main() parses the options into a Job and looks
// the run mode up in MODES; every mode is one function run_<mode>(const Job&) that returns the process's exit status:
//   infere / restart (:34-128, :369-385), test (:129-213), both (:214-283), pvals-calc (:284-368), predict / predict_single (:386-594);
//   [ext] ldscore (gv_ld_scores), clump (gv_ld_clump, section 20), score (section 21), screen (section 23 and,
//   with --cov-file, 26), pca (gv_pca_dev, section 24), king (gv_king_pairs, section 25), grm (gv_grm_pairs / gv_grm_block, section 28),
//   he (gv_grm_he, section 30).
// A new mode is one such function and one entry of MODES.  What the modes share sits above them: Job (the options every mode reads
// and the two ways to build a `data` from them), require_bed / require_one_rank, read_f64_file and Window (an LD window by kb, cM or
// marker count); driver_common.hpp holds what main_real_probit.cpp needs too.  Every mode is "load data, maybe run vamp::infere, one
// or more data::Ax, a reduction, a file": the matvecs are HIP kernels behind libgvamp, the rest is host code.  One process per GPU.
#include <algorithm>
#include <cmath>
#include <fstream>
#include <iostream>
#include <limits>
#include <sstream>

#include "data.hpp"
#include "driver_common.hpp"
#include "options.hpp"
#include "score_cols.hpp"
#include "utilities.hpp"
#include "vamp.hpp"

namespace {

struct Job {
    const Options& opt;
    const int rank = gv_env_rank();
    const std::string mode = opt.get_run_mode();
    const std::string type_data = opt.get_geno_format();      // [ext] --geno-format: "bed", or "dosage8" / "dosage16" code matrices
    const std::string bimfp = opt.get_bim_file();
    const int dev = opt.get_device(), km = opt.get_kernel_mode();
    const double alpha_scale = opt.get_alpha_scale(), dscale = opt.get_dosage_scale();
    const int dmiss = opt.get_dosage_missing();               // [ext] --dosage-missing: the all-ones code is a missing entry
    const int droute = opt.get_dosage_kernels() == "mfma" ? 1 : 0;      // [ext] --dosage-kernels: the route of the dosage products
    // [ext] --ld-dosage 1 with --cg-precond ld: the data object's context accepts the LD preconditioner on 8-bit codes (DESIGN.md
    // section 18).  Without the flag vamp::infere's refusal stands.
    const bool pcd = opt.get_ld_dosage() == 1 && opt.get_cg_precond() == "ld" && type_data != "bed";
    std::string out() const { return opt.get_out_dir() + opt.get_out_name(); }
    // a data object of this job's format and device on M of Mt markers from S on: phenotype file, or phenotype vector
    data load(const std::string& phenfp, const std::string& genofp, int N, int M, int Mt, int S) const {
        return data(phenfp, genofp, N, M, Mt, S, rank, type_data, alpha_scale, bimfp, dev, km, dscale, dmiss, droute);
    }
    data load(const std::vector<double>& y, const std::string& genofp, int N, int M, int Mt, int S) const {
        return data(y, genofp, N, M, Mt, S, rank, type_data, alpha_scale, bimfp, dev, km, dscale, dmiss, droute);
    }
};

// the end of a refusal whose message went to `os`: the failing exit status of the process, or the `false` of a check
int refuse(std::ostream& os) {
    os << std::endl;
    return EXIT_FAILURE;
}
bool unmet(std::ostream& os) { return refuse(os) == 0; }

bool require_bed(const Job& job) {
    return job.type_data == "bed" ||
           unmet(std::cout << "FATAL: --run-mode " << job.mode << " works on 2-bit genotypes only, not on --geno-format " << job.type_data);
}
bool require_one_rank(const Job& job, const char* reason) {
    return gv_env_nranks() <= 1 || unmet(std::cout << "FATAL: --run-mode " << job.mode << " runs on one rank: " << reason);
}

void opt_in_ld_dosage(const Job& job, data& ds) {
    if (job.pcd && gv_set_ld_dosage(ds.get_ctx(), 1)) exit(refuse(std::cout << "FATAL: gv_set_ld_dosage: " << gv_last_error(ds.get_ctx())));
}

// a whole file of `count` raw doubles, FATAL with both byte counts when it is short
bool read_f64_file(const std::string& file, const char* what, long long count, std::vector<double>& dst) {
    std::ifstream fp(file, std::ios::binary | std::ios::ate);
    if (!fp.is_open()) return unmet(std::cout << "FATAL: cannot open the " << what << " file " << file);
    const long long bytes = (long long)fp.tellg();
    if (bytes < 8LL * count)
        return unmet(std::cout << "FATAL: the " << what << " file " << file << " holds " << bytes << " bytes, fewer than the " << 8LL * count
                               << " of " << count << " float64 values");
    dst.assign((size_t)count, 0.0);
    fp.seekg(0);
    fp.read(reinterpret_cast<char*>(dst.data()), 8LL * count);
    return true;
}

// [ext] DESIGN.md section 19: an LD window by distance (kb of the base-pair column, cM of the cM column) or by marker count
struct Window {
    bool by_kb, by_cm;
    double kb;                  // the radius when by_kb
    const char* kb_flag;        // the option that names it: --ld-wind-kb, or --clump-kb
    bool has_positions(const Job& job) const {
        return !(by_kb || by_cm) || job.bimfp != "" ||
               unmet(std::cout << "FATAL: " << (by_kb ? kb_flag : "--ld-wind-cm") << " needs --bim-file: the positions are its "
                               << (by_kb ? "base-pair" : "cM") << " column");
    }
    // the positions and the radius: kb of the base-pair column, cM of the cM column, or the indices and --ld-window
    std::vector<double> positions(const Job& job, data& ds, int Mt, double* radius) const {
        std::vector<double> pos;
        *radius = (double)job.opt.get_ld_window();
        if (by_kb) {
            pos = ds.read_positions(job.bimfp, "bp");
            *radius = 1000.0 * kb;
        } else if (by_cm) {
            pos = ds.read_positions(job.bimfp, "cm");
            *radius = job.opt.get_ld_wind_cm();
        } else
            for (int j = 0; j < Mt; j++) pos.push_back((double)j);
        return pos;
    }
    void print(const Job& job) const {
        if (by_kb) std::cout << kb << " kb";
        else if (by_cm) std::cout << job.opt.get_ld_wind_cm() << " cM";
        else std::cout << job.opt.get_ld_window();
    }
};

// out-of-sample R2 of an estimate (main_real.cpp:163-176, :191-206): x_est * sqrt(N_test), one Ax, residual norm
double test_r2(data& ds, std::vector<double> x_est, int N_test, const std::vector<double>& y_test, double* err2_out,
               double intercept = 0.0, double scale = 1.0) {
    for (double& v : x_est) v *= sqrt((double)N_test);
    std::vector<double> z = ds.Ax(x_est.data());
    double err2 = 0;
    for (int i = 0; i < N_test; i++) {
        const double zi = intercept + scale * z[i];
        err2 += (y_test[i] - zi) * (y_test[i] - zi);
    }
    if (err2_out) *err2_out = err2;
    const double sd = calc_stdev(y_test);
    return 1 - err2 / (sd * sd * y_test.size());
}

double initial_gamw(const Options& opt) { return (opt.get_h2() == -1) ? 2 : 1.0 / (1.0 - opt.get_h2()); }   // :65-69

int run_infere(const Job& job) {                                                       // infere and restart
    const Options& opt = job.opt;
    const int Mt = (int)opt.get_Mt(), N = (int)opt.get_N();
    const auto [M, S] = shard_of(Mt);
    need_phen(opt.get_phen_files(), "--phen-files");
    data dataset = job.load(opt.get_phen_files()[0], opt.get_bed_file(), N, M, Mt, S);
    // infere: gam1 = 1e-6, gamw from --h2 (:64-69); restart: both from --gam1-init / --gamw-init (:381-382), r1 is
    // reloaded from --estimate-file inside infere_linear (vamp.cpp:226-233)
    const double gam1 = (job.mode == "restart") ? opt.get_gam1_init() : 1e-6;
    const double gamw = (job.mode == "restart") ? opt.get_gamw_init() : initial_gamw(opt);
    vamp emvamp(M, gam1, gamw, std::vector<double>(M, 0.0), job.rank, opt);
    opt_in_ld_dosage(job, dataset);
    infere_or_exit(emvamp, &dataset);
    return 0;
}

int run_test(const Job& job) {
    const Options& opt = job.opt;
    const int N_test = (int)opt.get_N_test(), Mt_test = (int)opt.get_Mt_test();
    const auto [M_test, S_test] = shard_of(Mt_test);
    need_phen(opt.get_phen_files_test(), "--phen-files-test");
    data dataset_test = job.load(opt.get_phen_files_test()[0], opt.get_bed_file_test(), N_test, M_test, Mt_test, S_test);
    std::vector<double> y_test = dataset_test.get_phen();
    const std::string est = opt.get_estimate_file();
    const size_t dot = est.find("."), pos_it = est.rfind("it");
    const std::string ext = est.substr(dot + 1);
    const std::vector<int> range = opt.get_test_iter_range();
    if (job.rank == 0) std::cout << "iter range = [" << range[0] << ", " << range[1] << "]" << std::endl;
    if (range[0] != -1) {                                                          // :152-181
        double maxR2 = -1;
        int maxind = -1;
        for (int it = range[0]; it <= range[1]; it++) {
            const std::string f = iteration_file(est, pos_it, ext, it);
            const double R2 = test_r2(dataset_test, load_estimate(f, M_test, S_test), N_test, y_test, nullptr);
            if (job.rank == 0) std::cout << R2 << ", ";
            if (R2 > maxR2) {
                maxR2 = R2;
                maxind = it;
            }
        }
        if (job.rank == 0)
            std::cout << std::endl << "max R2 = " << maxR2 << std::endl << std::endl << "max ind = " << maxind << std::endl;
    } else {                                                                       // :183-211
        if (job.rank == 0) std::cout << "est_file_name = " << est << std::endl;
        double err2 = 0;
        const double R2 = test_r2(dataset_test, load_estimate(est, M_test, S_test), N_test, y_test, &err2);
        const double sd = calc_stdev(y_test);
        if (job.rank == 0) {
            std::cout << "y stdev^2 = " << sd * sd << std::endl;
            std::cout << "test l2 pred err^2 = " << err2 << std::endl;
            std::cout << "test R2 = " << R2 << std::endl;
        }
    }
    return 0;
}

int run_both(const Job& job) {                                                         // :214-283
    const Options& opt = job.opt;
    const int Mt = (int)opt.get_Mt(), N = (int)opt.get_N();
    const auto [M, S] = shard_of(Mt);
    need_phen(opt.get_phen_files(), "--phen-files");
    need_phen(opt.get_phen_files_test(), "--phen-files-test");
    std::vector<double> x_est;
    double intercept, scale;
    {
        data dataset = job.load(opt.get_phen_files()[0], opt.get_bed_file(), N, M, Mt, S);
        vamp emvamp(M, 1e-6, initial_gamw(opt), std::vector<double>(M, 0.0), job.rank, opt);
        opt_in_ld_dosage(job, dataset);
        x_est = infere_or_exit(emvamp, &dataset);
        intercept = dataset.get_intercept();
        scale = dataset.get_scale();
    }
    if (job.rank == 0) std::cout << "intercept = " << intercept << std::endl << "scale = " << scale << std::endl;
    const int N_test = (int)opt.get_N_test(), Mt_test = (int)opt.get_Mt_test();
    data dataset_test = job.load(opt.get_phen_files_test()[0], opt.get_bed_file_test(), N_test, M, Mt_test, S);
    std::vector<double> y_test = dataset_test.get_phen();
    double err2 = 0;
    const double R2 = test_r2(dataset_test, x_est, N_test, y_test, &err2, intercept, scale);   // :262-272
    const double sd = calc_stdev(y_test);
    if (job.rank == 0) {
        std::cout << std::endl << "y stdev^2 = " << sd * sd << std::endl;
        std::cout << "test l2 pred err^2 = " << err2 << std::endl;
        std::cout << "test R2 = " << R2 << std::endl;
    }
    return 0;
}

int run_pvals_calc(const Job& job) {                                                   // :284-368
    const Options& opt = job.opt;
    const int Mt = (int)opt.get_Mt(), N = (int)opt.get_N();
    const Shard sh = shard_of(Mt);
    need_phen(opt.get_phen_files(), "--phen-files");
    data dataset = job.load(opt.get_phen_files()[0], opt.get_bed_file(), N, sh.M, Mt, sh.S);
    const std::string est = opt.get_estimate_file();
    const size_t dot = est.rfind("."), pos_it = est.rfind("it");
    const std::string ext = est.substr(dot + 1);
    const std::vector<int> range = opt.get_test_iter_range();
    if (job.rank == 0) std::cout << "iter range = [" << range[0] << ", " << range[1] << "]" << std::endl;
    std::vector<std::vector<double>> z1_hats, x1_hats;
    std::vector<std::string> out_loo, out_loco;
    const std::string pre = job.out();
    auto add = [&](const std::string& file, const std::string& tag) {
        std::vector<double> x = load_estimate(file, sh.M, sh.S);
        for (double& v : x) v *= sqrt((double)N);
        z1_hats.push_back(dataset.Ax(x.data()));
        x1_hats.push_back(x);
        out_loo.push_back(pre + tag + "_pvals.bin");
        out_loco.push_back(pre + tag);          // pvals_calc_LOCO appends "_pvals_LOCO.bin" (data.cpp:1347-1350)
    };
    if (range[0] != -1)
        for (int it = range[0]; it <= range[1]; it++) add(iteration_file(est, pos_it, ext, it), "_it_" + std::to_string(it));
    else
        add(est, "");
    std::vector<double> y = dataset.filter_pheno();
    const int sp = (int)opt.get_store_pvals();   // 0 = LOO and LOCO, 1 = only LOO, 2 = only LOCO (:313)
    if (sp == 0 || sp == 1) dataset.pvals_calc(z1_hats, y, x1_hats, out_loo);
    if (dataset.get_bimfp() != "" && (sp == 0 || sp == 2)) dataset.pvals_calc_LOCO(z1_hats, y, x1_hats, out_loco);
    return 0;
}

int run_ldscore(const Job& job) {                                                      // [ext] DESIGN.md section 16
    // LD scores of the markers over --ld-window markers on each side, among the individuals with a phenotype
    const Options& opt = job.opt;
    const bool ldd = job.type_data == "dosage8" && opt.get_ld_dosage() == 1;      // [ext] --ld-dosage 1: DESIGN.md section 17
    if (!ldd && !require_bed(job)) return EXIT_FAILURE;
    if (!require_one_rank(job, "the band stops at a shard's edges, so the scores of a sharded job would miss their neighbours across them"))
        return EXIT_FAILURE;
    // the window by distance (--ld-wind-kb / --ld-wind-cm) and the annotation categories (--ld-annot)
    const Window win{opt.get_ld_wind_kb() >= 0, opt.get_ld_wind_cm() >= 0, opt.get_ld_wind_kb(), "--ld-wind-kb"};
    const bool positional = win.by_kb || win.by_cm || opt.get_ld_annot() != "";
    if (opt.count_ld_windows() > 1) return refuse(std::cout << "FATAL: exactly one of --ld-window, --ld-wind-kb and --ld-wind-cm may be given");
    if (!win.has_positions(job)) return EXIT_FAILURE;
    const int Mt = (int)opt.get_Mt(), N = (int)opt.get_N();
    need_phen(opt.get_phen_files(), "--phen-files");
    data dataset = job.load(opt.get_phen_files()[0], opt.get_bed_file(), N, Mt, Mt, 0);
    if (ldd && gv_set_ld_dosage(dataset.get_ctx(), 1)) return refuse(std::cout << "FATAL: gv_set_ld_dosage: " << gv_last_error(dataset.get_ctx()));
    const std::string pre = job.out();
    gv_ld_stats st;
    if (!positional) {
        const std::vector<std::vector<double>> res = dataset.ld_scores_dev(opt.get_ld_window(), opt.get_ld_adjust() == 1);
        gv_ld_info(dataset.get_ctx(), &st);
        mpi_store_vec_to_file(pre + "_ldscore.bin", res[0], 0, Mt);
        mpi_store_vec_to_file(pre + "_ldscore_n.bin", res[1], 0, Mt);
        std::cout << "LD scores: window " << opt.get_ld_window() << (opt.get_ld_adjust() ? " (adjusted)" : "") << ", " << Mt << " markers, "
                  << st.seconds << " seconds" << std::endl;
        return 0;
    }
    double radius = 0.0;
    const std::vector<double> pos = win.positions(job, dataset, Mt, &radius);
    std::vector<std::string> cats;
    std::vector<double> annot;
    if (opt.get_ld_annot() != "") annot = dataset.read_annot(opt.get_ld_annot(), Mt, &cats);
    const int C = annot.empty() ? 1 : (int)cats.size();
    const std::vector<std::vector<double>> res = dataset.ld_scores_pos_dev(pos, radius, opt.get_ld_adjust() == 1, annot, C);
    gv_ld_info(dataset.get_ctx(), &st);
    mpi_store_vec_to_file(pre + "_ldscore.bin", res[0], 0, Mt * C);
    mpi_store_vec_to_file(pre + "_ldscore_n.bin", res[1], 0, Mt);
    if (!annot.empty()) {
        // the category sums over the polymorphic markers, and over those whose minor-allele frequency (mave / 2, folded to at
        // most 0.5) is above 0.05: what LD-score regression divides the heritability of a category by
        std::vector<double> tot(C, 0.0), tot5(C, 0.0);
        const double* mave = dataset.get_mave();
        for (int j = 0; j < Mt; j++) {
            if (res[1][j] == 0.0) continue;
            const double f = mave[j] / 2.0, maf = f > 0.5 ? 1.0 - f : f;
            for (int c = 0; c < C; c++) {
                tot[c] += annot[(size_t)j * C + c];
                if (maf > 0.05) tot5[c] += annot[(size_t)j * C + c];
            }
        }
        std::ofstream fm(pre + "_ldscore_M.txt"), fc(pre + "_ldscore_cats.txt");
        fm.precision(17);
        for (const std::vector<double>* t : {&tot, &tot5}) {
            for (int c = 0; c < C; c++) fm << (c ? " " : "") << (*t)[c];
            fm << "\n";
        }
        for (const std::string& nm : cats) fc << nm << "\n";
        if (!fm.good() || !fc.good()) return refuse(std::cout << "FATAL: cannot write " << pre << "_ldscore_M.txt / _ldscore_cats.txt");
    }
    std::cout << "LD scores: window ";
    win.print(job);
    std::cout << (opt.get_ld_adjust() ? " (adjusted)" : "") << ", " << Mt << " markers, " << C << (C == 1 ? " category, " : " categories, ")
              << st.seconds << " seconds" << std::endl;
    return 0;
}

int run_clump(const Job& job) {                                                        // [ext] DESIGN.md section 20
    // LD clumping of association results: the markers of p <= --clump-p1 in ascending p become index markers unless an earlier one
    // has claimed them; an index marker claims the markers of p <= --clump-p2 in its window with r^2 >= --clump-r2
    const Options& opt = job.opt;
    if (!require_bed(job)) return EXIT_FAILURE;
    if (!require_one_rank(job, "the band stops at a shard's edges, so the clumps of a sharded job would miss their members across them"))
        return EXIT_FAILURE;
    const bool given_kb = opt.get_clump_kb() >= 0 || opt.get_ld_wind_kb() >= 0;
    const int windows = opt.count_ld_windows() + (opt.get_clump_kb() >= 0 ? 1 : 0);
    if (windows > 1) return refuse(std::cout << "FATAL: exactly one of --clump-kb, --ld-wind-cm and --ld-window may be given");
    const double kb = opt.get_clump_kb() >= 0 ? opt.get_clump_kb() : (opt.get_ld_wind_kb() >= 0 ? opt.get_ld_wind_kb() : 250.0);
    const Window win{given_kb || windows == 0, opt.get_ld_wind_cm() >= 0, kb, "--clump-kb"};      // (no window given: --clump-kb 250)
    if (!win.has_positions(job)) return EXIT_FAILURE;
    const int Mt = (int)opt.get_Mt(), N = (int)opt.get_N();
    const std::string pfile = opt.get_clump_p_file();
    if (pfile == "")
        return refuse(std::cout << "FATAL: --run-mode clump needs --clump-p-file: " << Mt << " raw float64 p-values, the format of <out>_assoc_p.bin");
    std::vector<double> p;
    if (!read_f64_file(pfile, "p", Mt, p)) return EXIT_FAILURE;
    need_phen(opt.get_phen_files(), "--phen-files");
    data dataset = job.load(opt.get_phen_files()[0], opt.get_bed_file(), N, Mt, Mt, 0);
    double radius = 0.0;
    const std::vector<double> pos = win.positions(job, dataset, Mt, &radius);
    // the marker ids and chromosomes of the report: columns 2 and 1 of the .bim file, or m<j> and 0 without one
    std::vector<std::string> ids, chr;
    if (job.bimfp != "") {
        std::ifstream fb(job.bimfp);
        std::string c1, c2, line;
        while ((int)ids.size() < Mt && getline(fb, line)) {
            std::istringstream ls(line);
            ls >> c1 >> c2;
            chr.push_back(c1);
            ids.push_back(c2);
        }
    }
    for (int j = (int)ids.size(); j < Mt; j++) {
        ids.push_back("m" + std::to_string(j));
        chr.push_back("0");
    }
    int64_t n_index = 0;
    const std::vector<int64_t> index_of =
        dataset.ld_clump_dev(pos, radius, p, opt.get_clump_p1(), opt.get_clump_p2(), opt.get_clump_r2(), &n_index);
    gv_ld_stats st;
    gv_ld_info(dataset.get_ctx(), &st);
    int rounds = 0;
    gv_ld_clump_last(dataset.get_ctx(), &rounds, nullptr, nullptr);
    const std::string pre = job.out();
    mpi_store_vec_to_file(pre + "_clump_index.bin", std::vector<double>(index_of.begin(), index_of.end()), 0, Mt);
    // one line per clump, in the order the index markers were chosen (ascending p, ties by index): the index marker's id, chromosome,
    // position and p, the number of markers it claimed and their ids
    std::vector<int> lead;
    std::vector<std::vector<int>> members((size_t)Mt);
    for (int j = 0; j < Mt; j++) {
        if (index_of[j] == j) lead.push_back(j);
        else if (index_of[j] >= 0) members[(size_t)index_of[j]].push_back(j);
    }
    std::stable_sort(lead.begin(), lead.end(), [&](int x, int y) { return p[x] < p[y]; });
    std::ofstream fc(pre + "_clumps.txt");
    fc.precision(17);
    for (int j : lead) {
        fc << ids[j] << " " << chr[j] << " " << pos[j] << " " << p[j] << " " << members[j].size();
        for (size_t t = 0; t < members[j].size(); t++) fc << (t ? "," : " ") << ids[members[j][t]];
        fc << "\n";
    }
    fc.close();
    if (!fc.good()) return refuse(std::cout << "FATAL: cannot write " << pre << "_clumps.txt");
    std::cout << "LD clumping: window ";
    win.print(job);
    std::cout << ", p1 " << opt.get_clump_p1() << ", p2 " << opt.get_clump_p2() << ", r2 " << opt.get_clump_r2() << ", " << Mt << " markers, "
              << st.seconds << " seconds, " << n_index << " clumps, " << rounds << " rounds, " << st.block_pairs << " blocks launched"
              << std::endl;
    return 0;
}

int run_score(const Job& job) {                                                        // [ext] DESIGN.md section 21
    // many weight vectors applied to a cohort in one go: <out>_scores.bin = C columns of N float64
    const Options& opt = job.opt;
    const int N_test = (int)opt.get_N_test(), Mt_test = (int)opt.get_Mt_test();
    const long long C0 = (long long)opt.get_score_cols();
    const std::string sfile = opt.get_score_file(), units = opt.get_score_units();
    const std::vector<double>& thr = opt.get_score_p_thresholds();
    const bool ct = !thr.empty() || opt.get_score_clump_index() != "" || opt.get_score_p_file() != "";
    if (sfile == "")
        return refuse(std::cout << "FATAL: --run-mode score needs --score-file: --score-cols x " << Mt_test << " raw float64 weights, column after column");
    if (ct && (thr.empty() || opt.get_score_clump_index() == "" || opt.get_score_p_file() == ""))
        return refuse(std::cout << "FATAL: --score-clump-index, --score-p-file and --score-p-thresholds go together: all three or none");
    if (ct && C0 != 1)
        return refuse(std::cout << "FATAL: --score-p-thresholds builds its columns from column 0 of the score file: it needs --score-cols 1, not " << C0);
    std::vector<double> wall, pall, iall;
    if (!read_f64_file(sfile, "score", C0 * Mt_test, wall)) return EXIT_FAILURE;
    if (ct && (!read_f64_file(opt.get_score_p_file(), "p", Mt_test, pall) || !read_f64_file(opt.get_score_clump_index(), "clump index", Mt_test, iall)))
        return EXIT_FAILURE;
    const auto [M_test, S_test] = shard_of(Mt_test);
    data dataset_test = job.load(std::vector<double>(N_test, 0.0), opt.get_bed_file_test(), N_test, M_test, Mt_test, S_test);
    // this shard's slice of every column
    std::vector<std::vector<double>> cols;
    if (ct) {
        // (index_of is global in the file; a marker is an index marker iff it names itself, which a shard-local index keeps)
        std::vector<int64_t> idx((size_t)M_test);
        for (int j = 0; j < M_test; j++) {
            const double g = iall[(size_t)S_test + j];
            idx[(size_t)j] = g == (double)(S_test + j) ? (int64_t)j : (g < 0 ? -1 : (int64_t)M_test + 1);
        }
        cols = score_cols::threshold_columns(wall.data() + S_test, idx.data(), pall.data() + S_test, (size_t)M_test, thr);
    } else
        for (long long k = 0; k < C0; k++)
            cols.emplace_back(wall.begin() + k * Mt_test + S_test, wall.begin() + k * Mt_test + S_test + M_test);
    const size_t C = cols.size();
    const double sqrtN = sqrt((double)N_test);
    std::vector<double> konst(C, 0.0);
    for (size_t k = 0; k < C; k++) {
        if (units == "allele") {
            konst[k] = score_cols::allele_constant(cols[k].data(), dataset_test.get_mave(), (size_t)M_test);
            cols[k] = score_cols::allele_to_std(cols[k].data(), dataset_test.get_msig(), (size_t)M_test, sqrtN);
        } else
            for (double& v : cols[k]) v *= sqrtN;                                    // as predict scales an estimate
    }
    if (units == "allele" && gv_env_nranks() > 1 && gv_allreduce_host(dataset_test.get_ctx(), konst.data(), (int)C))
        return refuse(std::cout << "FATAL: gv_allreduce_host: " << gv_last_error(dataset_test.get_ctx()));
    std::vector<std::vector<double>> z = dataset_test.score(cols);
    gv_score_stats st;
    gv_score_info(dataset_test.get_ctx(), &st);
    const std::string pre = job.out();
    if (job.rank == 0) {
        std::ofstream fo(pre + "_scores.bin", std::ios::binary);
        for (size_t k = 0; k < C; k++) {
            if (units == "allele")
                for (int i = 0; i < N_test; i++) z[k][(size_t)i] += konst[k];
            fo.write(reinterpret_cast<const char*>(z[k].data()), 8LL * N_test);
        }
        fo.close();
        if (!fo.good()) return refuse(std::cout << "FATAL: cannot write " << pre << "_scores.bin");
        std::cout << "scores: " << C << " columns (" << units << " units) x " << N_test << " individuals, "
                  << (st.path == GV_SCORE_PATH_KERNEL ? "kernel" : "fallback") << " path, " << st.passes << " passes, " << st.seconds
                  << " seconds -> " << pre << "_scores.bin" << std::endl;
    }
    return 0;
}

// the phenotype matrix of the screen and its complete cases
struct Phenotypes {
    std::vector<std::vector<double>> Y;      // column c = the third token of every line of file c, NA -> NaN
    std::vector<char> have;                  // individual n has a value in every file (and, later, every covariate)
    std::vector<unsigned char> m4;           // the same as a 4-bit mask
    int nonas = 0;
};

// complete cases: an individual with NA in any file is masked
bool read_phenotypes(const std::vector<std::string>& files, int N, Phenotypes& ph) {
    ph.Y.resize(files.size());
    ph.m4.assign((size_t)(N + 3) / 4, 0);
    ph.have.assign((size_t)N, 1);
    for (size_t c = 0; c < files.size(); c++) {
        std::ifstream in(files[c]);
        if (!in.is_open()) return unmet(std::cout << "FATAL: could not open phenotype file: " << files[c]);
        std::string line;
        while (getline(in, line)) {
            std::istringstream ls(line);
            std::string a, b, v;
            if (!(ls >> a >> b >> v)) return unmet(std::cout << "FATAL: phenotype line with fewer than 3 columns in " << files[c]);
            ph.Y[c].push_back(v == "NA" ? std::numeric_limits<double>::quiet_NaN() : atof(v.c_str()));
        }
        if ((int)ph.Y[c].size() != N) return unmet(std::cout << "FATAL: " << files[c] << " holds " << ph.Y[c].size() << " lines, not --N = " << N);
        for (int n = 0; n < N; n++)
            if (std::isnan(ph.Y[c][(size_t)n])) ph.have[(size_t)n] = 0;
    }
    for (int n = 0; n < N; n++)
        if (ph.have[(size_t)n]) {
            ph.m4[(size_t)n / 4] |= (unsigned char)(1u << (n % 4));
            ph.nonas++;
        }
    return true;
}

// the tags of the screen's output files, and what every path of it needs
const char* const SCREEN_TAG[5] = {"_screen_r.bin", "_screen_t.bin", "_screen_p.bin", "_screen_beta.bin", "_screen_se.bin"};
struct Screen {
    const Job& job;
    data& dataset;
    Phenotypes& ph;      // (read_covariate_cases takes individuals out of it)
    int N, Mt;
    Shard sh;

    // the phenotypes in blocks of --screen-cols columns: one(block) returns ntag result vectors of one column per phenotype, and
    // column c of vector k goes to value c * Mt + S of <out><tag k>
    template <class F>
    void blocks(int ntag, F one) const {
        const size_t C = ph.Y.size(), per = job.opt.get_screen_cols();
        for (size_t c0 = 0; c0 < C; c0 += per) {
            const size_t c1 = c0 + per < C ? c0 + per : C;
            const auto res = one(std::vector<std::vector<double>>(ph.Y.begin() + c0, ph.Y.begin() + c1));
            for (int k = 0; k < ntag; k++)
                for (size_t c = c0; c < c1; c++)
                    mpi_store_vec_to_file(job.out() + SCREEN_TAG[k], res[(size_t)k][c - c0], (int)(c * (size_t)Mt) + sh.S, sh.M);
        }
    }
};

int screen_plain(const Screen& s) {
    long long passes = 0;
    double seconds = 0.0;
    gv_atxm_stats st{};
    s.blocks(3, [&](const std::vector<std::vector<double>>& blk) {
        const auto res = s.dataset.screen(blk);
        gv_atxm_info(s.dataset.get_ctx(), &st);
        passes += st.passes;
        seconds += st.seconds;
        return res;
    });
    if (s.job.rank == 0)
        std::cout << "screen: " << s.ph.Y.size() << " phenotypes x " << s.Mt << " markers, " << s.ph.nonas << " complete cases of " << s.N << ", "
                  << (st.path == GV_ATXM_PATH_KERNEL ? "kernel" : "fallback") << " path, " << passes << " passes, " << seconds
                  << " seconds -> " << s.job.out() << "_screen_{r,t,p}.bin" << std::endl;
    return 0;
}

// [ext] --cov-file F --C K: the screen adjusted for K covariates and an intercept
int screen_adjusted(const Screen& s, int K) {
    s.dataset.screen_cov_set();
    gv_screen_cov_stats cs{};
    gv_screen_cov_info(s.dataset.get_ctx(), &cs);
    double prod = 0.0, panel = 0.0;
    s.blocks(5, [&](const std::vector<std::vector<double>>& blk) {
        const auto res = s.dataset.screen_cov(blk, s.job.opt.get_screen_vif());
        gv_screen_cov_info(s.dataset.get_ctx(), &cs);
        prod += cs.call_seconds_products;
        panel += cs.call_seconds_panel;
        return res;
    });
    if (s.job.rank == 0)
        std::cout << "screen: " << s.ph.Y.size() << " phenotypes x " << s.Mt << " markers adjusted for " << K << " covariates, " << s.ph.nonas
                  << " complete cases of " << s.N << ", nu = " << cs.nu << ", set " << cs.set_seconds << " seconds, products " << prod
                  << " s, panel and finishing kernels " << panel << " s -> " << s.job.out() << "_screen_{r,t,p,beta,se}.bin" << std::endl;
    return 0;
}

// the K covariates of --cov-file: complete cases over the phenotype files and the covariates
bool read_covariate_cases(const Screen& s, int K) {
    if (K < 1 || K > GV_PCA_MAX_BLOCK)
        return unmet(std::cout << "FATAL: --run-mode screen --cov-file needs --C K, the number of covariates per line (1.." << GV_PCA_MAX_BLOCK << ")");
    s.dataset.read_covariates(s.job.opt.get_cov_file(), K);
    const std::vector<std::vector<double>> Z = s.dataset.get_covs();
    for (int n = 0; n < s.N; n++) {
        bool fin = true;
        for (int k = 0; k < K; k++) fin = fin && std::isfinite(Z[(size_t)n][(size_t)k]);
        if (!fin && s.ph.have[(size_t)n]) {
            s.ph.have[(size_t)n] = 0;
            s.ph.m4[(size_t)n / 4] &= (unsigned char)~(1u << (n % 4));
            s.ph.nonas--;
        }
    }
    return s.ph.nonas - 2 - K >= 1 || unmet(std::cout << "FATAL: --run-mode screen: " << s.ph.nonas << " complete cases and " << K
                                                      << " covariates leave the test no degree of freedom");
}

int run_screen(const Job& job) {                                                       // [ext] DESIGN.md section 23
    // every phenotype file against every marker: <out>_screen_{r,t,p}.bin = C columns of Mt float64
    const Options& opt = job.opt;
    // [ext] --screen-dosage 1: dosage codes pass; without it the refusal stands
    const bool dosage = opt.get_screen_dosage() == 1 && (job.type_data == "dosage8" || job.type_data == "dosage16");
    if (!dosage && !require_bed(job)) return EXIT_FAILURE;
    const int Mt = (int)opt.get_Mt(), N = (int)opt.get_N();
    const Shard sh = shard_of(Mt);
    need_phen(opt.get_phen_files(), "--phen-files");
    const size_t C = opt.get_phen_files().size();
    if ((long long)C * Mt > 2147483647LL)
        return refuse(std::cout << "FATAL: --run-mode screen: " << C << " columns x " << Mt << " markers exceed the 2^31 - 1 values of an output file");
    Phenotypes ph;
    if (!read_phenotypes(opt.get_phen_files(), N, ph)) return EXIT_FAILURE;
    if (ph.nonas < 3) return refuse(std::cout << "FATAL: --run-mode screen: " << ph.nonas << " complete cases leave the test no degree of freedom");
    data dataset = job.load(std::vector<double>(N, 0.0), opt.get_bed_file(), N, sh.M, Mt, sh.S);
    if (dosage && gv_set_screen_dosage(dataset.get_ctx(), 1))
        return refuse(std::cout << "FATAL: gv_set_screen_dosage: " << gv_last_error(dataset.get_ctx()));
    const Screen s{job, dataset, ph, N, Mt, sh};
    const bool with_cov = opt.get_cov_file() != "";
    if (with_cov && !read_covariate_cases(s, (int)opt.get_C())) return EXIT_FAILURE;
    dataset.set_mask(ph.m4, ph.nonas);
    return with_cov ? screen_adjusted(s, (int)opt.get_C()) : screen_plain(s);
}

int run_pca(const Job& job) {                                                          // [ext] DESIGN.md section 24
    // the K leading principal components of the standardised genotypes among the individuals with a phenotype
    const Options& opt = job.opt;
    const int Mt = (int)opt.get_Mt(), N = (int)opt.get_N();
    const int K = (int)opt.get_pca_k();
    if (K < 1)
        return refuse(std::cout << "FATAL: --run-mode pca needs --pca-k K, the number of principal components (1.." << GV_PCA_MAX_BLOCK << ")");
    const int L = opt.get_pca_block() ? (int)opt.get_pca_block() : std::min(GV_PCA_MAX_BLOCK, K + std::max(8, K));
    if (L < K || L > GV_PCA_MAX_BLOCK)
        return refuse(std::cout << "FATAL: --run-mode pca: the block has to hold --pca-k = " << K << " vectors and at most " << GV_PCA_MAX_BLOCK
                                << " (--pca-block " << L << ")");
    if ((long long)K * Mt > 2147483647LL)
        return refuse(std::cout << "FATAL: --run-mode pca: " << K << " columns x " << Mt << " markers exceed the 2^31 - 1 values of an output file");
    const auto [M, S] = shard_of(Mt);
    need_phen(opt.get_phen_files(), "--phen-files");
    data dataset = job.load(opt.get_phen_files()[0], opt.get_bed_file(), N, M, Mt, S);
    const data::pca_result res = dataset.pca(K, L, opt.get_pca_tol(), (int)opt.get_pca_max_iter(), opt.get_pca_seed(), true);
    const std::string pre = job.out();
    double worst = 0.0;
    for (int i = 0; i < K; i++) worst = std::max(worst, res.resid[(size_t)i] / res.eval[(size_t)i]);
    if (!res.info.converged) {
        // eigenvectors that missed the tolerance are not covariates anybody asked for: nothing is written unless the caller says so
        const bool allow = opt.get_pca_allow_unconverged() == 1;
        std::cout << (allow ? "WARNING" : "FATAL") << ": --run-mode pca: NOT converged after " << res.info.iterations
                  << " iterations (largest r / theta = " << worst << ", --pca-tol " << opt.get_pca_tol() << ")"
                  << (allow ? ": the files hold the last Ritz pairs (--pca-allow-unconverged 1)"
                            : ": nothing written; raise --pca-max-iter or --pca-block, or pass --pca-allow-unconverged 1")
                  << std::endl;
        if (!allow) return EXIT_FAILURE;
    }
    // column i of the loadings starts at value i * Mt of the file: within an int by the K * Mt check above
    for (int i = 0; i < K; i++) mpi_store_vec_to_file(pre + "_pca_loadings.bin", res.loadings[(size_t)i], (int)((size_t)i * (size_t)Mt) + S, M);
    if (job.rank == 0) {                                   // N-space is the same on every rank
        FILE* fv = fopen((pre + "_pca_eigenval.txt").c_str(), "w");
        FILE* fu = fopen((pre + "_pca_eigenvec.txt").c_str(), "w");
        bool ok = fv && fu;
        for (int i = 0; i < K && ok; i++) ok = fprintf(fv, "%.17g\n", res.eval[(size_t)i]) > 0;
        for (int n = 0; n < N && ok; n++)
            for (int i = 0; i < K && ok; i++) ok = fprintf(fu, i + 1 < K ? "%.17g " : "%.17g\n", res.evec[(size_t)i][(size_t)n]) > 0;
        if (fv) ok = fclose(fv) == 0 && ok;
        if (fu) ok = fclose(fu) == 0 && ok;
        if (!ok) return refuse(std::cout << "FATAL: cannot write " << pre << "_pca_eigenval.txt / _pca_eigenvec.txt");
        std::cout << "pca: " << K << " components of " << N << " individuals x " << Mt << " markers, block " << L << ", "
                  << res.info.iterations << " iterations, " << (res.info.converged ? "converged" : "NOT converged") << " (largest r / theta = "
                  << worst << ", tol " << opt.get_pca_tol() << "), products " << res.info.seconds_products << " s, panel kernels "
                  << res.info.seconds_panel << " s -> " << pre << "_pca_{eigenval.txt,eigenvec.txt,loadings.bin}" << std::endl;
    }
    return 0;
}

int run_king(const Job& job) {                                                         // [ext] DESIGN.md section 25
    // the pairs of individuals at or above a kinship cutoff, from the genotypes alone: no phenotype file
    const Options& opt = job.opt;
    if (!require_bed(job)) return EXIT_FAILURE;
    if (!require_one_rank(job, "the counts of a pair are sums over the markers of all ranks, and the integer all-reduce that would add "
                               "them is not built"))
        return EXIT_FAILURE;
    const int Mt = (int)opt.get_Mt(), N = (int)opt.get_N();
    std::vector<unsigned char> use;
    if (opt.get_king_marker_file() != "") {
        std::ifstream in(opt.get_king_marker_file(), std::ios::binary);
        use.assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
        if (!in.is_open() || use.size() != (size_t)Mt)
            return refuse(std::cout << "FATAL: --king-marker-file " << opt.get_king_marker_file() << " must hold Mt = " << Mt << " bytes of 0 / 1 ("
                                    << (in.is_open() ? std::to_string(use.size()) + " bytes read" : std::string("cannot open it")) << ")");
    }
    setenv("GVAMP_RESIDENT_LAYOUT", "2", 0);      // the kernel reads the tile layout (a --resident-layout given on the command line stands)
    data dataset = job.load(std::vector<double>(N, 0.0), opt.get_bed_file(), N, Mt, Mt, 0);      // (bed data: the dosage arguments are unused)
    const data::king_result res = dataset.king_pairs(opt.get_king_cutoff(), use);
    const std::string path = job.out() + "_king.kin0.txt";
    FILE* f = fopen(path.c_str(), "w");
    bool ok = f != nullptr;
    for (size_t t = 0; t < res.i.size() && ok; t++) {
        const int32_t* q = &res.counts[5 * t];
        ok = fprintf(f, "%d %d %d %d %d %d %d %.17g\n", res.i[t], res.j[t], q[0], q[1], q[2], q[3], q[4], res.kin[t]) > 0;
    }
    if (f) ok = fclose(f) == 0 && ok;
    if (!ok) return refuse(std::cout << "FATAL: cannot write " << path);
    std::cout << "king: " << N << " individuals x " << res.info.used_markers << " of " << Mt << " markers, cutoff " << opt.get_king_cutoff()
              << ": " << res.i.size() << " pairs, " << res.info.seconds << " seconds -> " << path << std::endl;
    return 0;
}

// <out>.grm.sp: GCTA's sparse text -- the N diagonal entries by row, then the pairs at or above the cutoff in ascending (i, j)
int grm_sparse(const Job& job, data& dataset, const std::vector<unsigned char>& use, int N, int Mt) {
    const data::grm_result res = dataset.grm_pairs(job.opt.get_grm_cutoff(), use);
    const std::string path = job.out() + ".grm.sp";
    FILE* f = fopen(path.c_str(), "w");
    bool ok = f != nullptr;
    for (int n = 0; n < N && ok; n++) ok = fprintf(f, "%d %d %.17g\n", n, n, res.diag[(size_t)n]) > 0;
    for (size_t t = 0; t < res.i.size() && ok; t++) ok = fprintf(f, "%d %d %.17g\n", res.i[t], res.j[t], res.a[t]) > 0;
    if (f) ok = fclose(f) == 0 && ok;
    if (!ok) return refuse(std::cout << "FATAL: cannot write " << path);
    std::cout << "grm: " << N << " individuals x " << res.info.counting_markers << " counting of " << Mt << " markers ("
              << res.info.dropped_markers << " dropped as monomorphic or never present), cutoff " << job.opt.get_grm_cutoff() << ": "
              << res.i.size() << " pairs, " << res.info.seconds << " seconds -> " << path << std::endl;
    return 0;
}

// <out>.grm.bin / <out>.grm.N.bin: GCTA's dense format -- the lower triangle with the diagonal, row by row, as float32; streamed in row
// panels [r0, r0 + P) x [0, r0 + P), so that N^2 doubles never sit on the host
int grm_dense(const Job& job, data& dataset, const std::vector<unsigned char>& use, int N, int Mt) {
    const std::string pa = job.out() + ".grm.bin", pn = job.out() + ".grm.N.bin";
    FILE *fa = nullptr, *fn = nullptr;              // (opened after the first panel: a refused call leaves no file behind)
    bool ok = true;
    const int64_t P = std::max<int64_t>(64, std::min<int64_t>(N, ((int64_t)1 << 25) / N / 64 * 64));      // at most 2^25 entries a panel
    double seconds = 0.0;
    gv_grm_stats info{};
    std::vector<float> row;
    for (int64_t r0 = 0; r0 < N && ok; r0 += P) {
        const int64_t nr = std::min<int64_t>(P, N - r0), nc = r0 + nr;
        const data::grm_result res = dataset.grm_block(r0, nr, 0, nc, use);
        info = res.info;
        seconds += res.info.seconds;
        if (r0 == 0) {
            fa = fopen(pa.c_str(), "wb");
            fn = fopen(pn.c_str(), "wb");
            ok = fa && fn;
        }
        for (int64_t r = 0; r < nr && ok; r++) {
            const size_t len = (size_t)(r0 + r + 1);
            row.resize(len);
            for (size_t k = 0; k < len; k++) row[k] = (float)res.a[(size_t)r * (size_t)nc + k];
            ok = fwrite(row.data(), sizeof(float), len, fa) == len;
            for (size_t k = 0; k < len; k++) row[k] = (float)res.m_common[(size_t)r * (size_t)nc + k];
            ok = ok && fwrite(row.data(), sizeof(float), len, fn) == len;
        }
    }
    if (fa) ok = fclose(fa) == 0 && ok;
    if (fn) ok = fclose(fn) == 0 && ok;
    if (!ok) return refuse(std::cout << "FATAL: cannot write " << pa << " / " << pn);
    std::cout << "grm: " << N << " individuals x " << info.counting_markers << " counting of " << Mt << " markers (" << info.dropped_markers
              << " dropped as monomorphic or never present), dense: " << (int64_t)N * (N + 1) / 2 << " pairs, " << seconds << " seconds -> "
              << pa << ", " << pn << std::endl;
    return 0;
}

int run_grm(const Job& job) {                                                          // [ext] DESIGN.md section 28
    // the standardised genetic relationship matrix, from the genotypes alone: no phenotype file
    const Options& opt = job.opt;
    if (!require_bed(job)) return EXIT_FAILURE;
    if (!require_one_rank(job, "S and the common-marker count of a pair are sums over the markers of all ranks, and the all-reduce that "
                               "would add them is not built"))
        return EXIT_FAILURE;
    const int Mt = (int)opt.get_Mt(), N = (int)opt.get_N();
    std::vector<unsigned char> use;
    if (opt.get_grm_marker_file() != "") {
        std::ifstream in(opt.get_grm_marker_file(), std::ios::binary);
        use.assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
        if (!in.is_open() || use.size() != (size_t)Mt)
            return refuse(std::cout << "FATAL: --grm-marker-file " << opt.get_grm_marker_file() << " must hold Mt = " << Mt << " bytes of 0 / 1 ("
                                    << (in.is_open() ? std::to_string(use.size()) + " bytes read" : std::string("cannot open it")) << ")");
    }
    setenv("GVAMP_RESIDENT_LAYOUT", "2", 0);      // the kernel reads the tile layout (a --resident-layout given on the command line stands)
    data dataset = job.load(std::vector<double>(N, 0.0), opt.get_bed_file(), N, Mt, Mt, 0);      // (bed data: the dosage arguments are unused)
    return opt.get_grm_has_cutoff() ? grm_sparse(job, dataset, use, N, Mt) : grm_dense(job, dataset, use, N, Mt);
}

int run_he(const Job& job) {                                                           // [ext] DESIGN.md section 30
    // Haseman-Elston regression of every phenotype file on the relationship matrix, which is never stored
    const Options& opt = job.opt;
    if (!require_bed(job)) return EXIT_FAILURE;
    if (!require_one_rank(job, "S and the common-marker count of a pair are sums over the markers of all ranks, and the all-reduce that "
                               "would add them is not built"))
        return EXIT_FAILURE;
    const int Mt = (int)opt.get_Mt(), N = (int)opt.get_N();
    need_phen(opt.get_phen_files(), "--phen-files");
    const std::vector<std::string>& files = opt.get_phen_files();
    Phenotypes ph;                                  // (every trait keeps its own missing set: the complete cases are not used)
    if (!read_phenotypes(files, N, ph)) return EXIT_FAILURE;
    std::vector<unsigned char> use;
    if (opt.get_grm_marker_file() != "") {
        std::ifstream in(opt.get_grm_marker_file(), std::ios::binary);
        use.assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
        if (!in.is_open() || use.size() != (size_t)Mt)
            return refuse(std::cout << "FATAL: --grm-marker-file " << opt.get_grm_marker_file() << " must hold Mt = " << Mt << " bytes of 0 / 1 ("
                                    << (in.is_open() ? std::to_string(use.size()) + " bytes read" : std::string("cannot open it")) << ")");
    }
    const size_t C = files.size();
    std::vector<double> y((size_t)N * C);
    for (size_t c = 0; c < C; c++)
        for (int n = 0; n < N; n++) y[(size_t)n * C + c] = ph.Y[c][(size_t)n];
    setenv("GVAMP_RESIDENT_LAYOUT", "2", 0);      // the kernel reads the tile layout (a --resident-layout given on the command line stands)
    data dataset = job.load(std::vector<double>(N, 0.0), opt.get_bed_file(), N, Mt, Mt, 0);      // (bed data: the dosage arguments are unused)
    const data::grm_he_result res = dataset.grm_he((int64_t)C, y, use);
    const std::string path = job.out() + ".HEreg";
    FILE* f = fopen(path.c_str(), "w");
    bool ok = f != nullptr && fprintf(f, "trait n_ind n_pairs mean_a var_a h2 intercept se_ols se_jack\n") > 0;
    for (size_t c = 0; c < C && ok; c++) {
        const gv_he_result& r = res.traits[c];
        const double mean = r.sum_a / (double)r.n_pairs, var = r.sum_aa / (double)r.n_pairs - mean * mean;
        ok = fprintf(f, "%s %lld %lld %.17g %.17g %.17g %.17g %.17g %.17g\n", files[c].c_str(), (long long)r.n_ind, (long long)r.n_pairs, mean,
                     var, r.h2, r.intercept, r.se_ols, r.se_jack) > 0;
    }
    if (f) ok = fclose(f) == 0 && ok;
    if (!ok) return refuse(std::cout << "FATAL: cannot write " << path);
    std::cout << "he: " << N << " individuals x " << res.info.counting_markers << " counting of " << Mt << " markers, " << C << " traits, "
              << res.info.passes << " passes, " << res.info.blocks_computed << " blocks, " << res.info.seconds << " seconds -> " << path
              << std::endl;
    return 0;
}

int run_predict(const Job& job) {                                                      // predict and predict_single (:386-594)
    const Options& opt = job.opt;
    const int N_test = (int)opt.get_N_test(), Mt_test = (int)opt.get_Mt_test();
    const Shard sh = shard_of(Mt_test);
    data dataset_test = job.load(std::vector<double>(N_test, 0.0), opt.get_bed_file_test(), N_test, sh.M, Mt_test, sh.S);
    const std::string est = opt.get_estimate_file();
    const std::string ext = est.substr(est.find(".") + 1);
    const std::string pre = job.out();
    auto predict = [&](const std::string& file) {
        std::vector<double> x = load_estimate(file, sh.M, sh.S);
        for (double& v : x) v *= sqrt((double)N_test);
        return dataset_test.Ax(x.data());
    };
    if (job.mode == "predict_single") {
        std::vector<double> z = predict(est);
        if (job.rank == 0) {
            std::cout << "filepath_out = " << pre + "_predict.csv" << std::endl;
            store_vec_to_file(pre + "_predict.csv", z);
        }
        return 0;
    }
    if (job.rank == 0) std::cout << "est_file_name = " << est << std::endl;
    const size_t pos_it = est.rfind("temp");
    const std::vector<int> range = opt.get_test_iter_range();
    if (job.rank == 0) std::cout << "iter range = [" << range[0] << ", " << range[1] << "]" << std::endl;
    if (range[0] != -1) {
        std::vector<std::vector<double>> zs;
        for (int it = range[0]; it <= range[1]; it++) {
            const std::string f = est.substr(0, pos_it) + "temp_" + std::to_string(it) + "_" + std::to_string(it) +
                                  "_gibbs_est." + ext;
            if (job.rank == 0) std::cout << "est_file_name_it = " << f << std::endl;
            zs.push_back(predict(f));
        }
        for (int i = 0; i < N_test && job.rank == 0; i++) {       // one csv per individual (:424-434)
            std::vector<double> row;
            for (auto& z : zs) row.push_back(z[i]);
            store_vec_to_file(pre + "_predict_" + std::to_string(i) + ".csv", row);
        }
    }
    return 0;
}

const struct {
    const char* name;
    int (*run)(const Job&);
} MODES[] = {{"infere", run_infere}, {"restart", run_infere}, {"test", run_test}, {"both", run_both}, {"pvals-calc", run_pvals_calc},
             {"predict", run_predict}, {"predict_single", run_predict}, {"ldscore", run_ldscore}, {"clump", run_clump},
             {"score", run_score}, {"screen", run_screen}, {"pca", run_pca}, {"king", run_king}, {"grm", run_grm}, {"he", run_he}};

}  // namespace

int main(int argc, char** argv) {
    const Options opt(argc, argv);
    const Job job{opt};
    if (job.dmiss && job.type_data == "bed" && job.rank == 0)
        std::cout << "WARNING: --dosage-missing is ignored for --geno-format bed (PLINK rows carry their own missing code)" << std::endl;
    if (opt.get_screen_dosage() && job.type_data == "bed" && job.rank == 0)
        std::cout << "WARNING: --screen-dosage is ignored for --geno-format bed (the screen of 2-bit genotypes needs no option)" << std::endl;
    if (job.droute && job.type_data == "bed" && job.rank == 0)
        std::cout << "WARNING: --dosage-kernels is ignored for --geno-format bed (gv_set_kernel_mode selects the bed kernels)" << std::endl;
    if (job.pcd && (job.mode == "infere" || job.mode == "restart" || job.mode == "both") && job.type_data != "dosage8")
        return refuse(std::cout << "FATAL: --cg-precond ld with --ld-dosage 1 covers --geno-format dosage8 only, not --geno-format " << job.type_data);
    for (const auto& m : MODES)
        if (job.mode == m.name) {
            const int status = m.run(job);
            if (status == 0) gv_host_finalize();      // the process's communicator, after the last data object (MPI_Finalize of the reference)
            return status;
        }
    return refuse(std::cout << "FATAL: unknown --run-mode \"" << job.mode << "\"");
}
