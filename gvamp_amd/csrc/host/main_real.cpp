// main_real.cpp -- real-data driver mirroring the reference's main_real.cpp:13-599, all run modes:
//   infere (:34-128), test (:129-213), both (:214-283), pvals-calc (:284-368), restart (:369-385),
//   predict (:386-437), predict_single (:438-594); [ext] ldscore (gv_ld_scores), clump (gv_ld_clump, section 20),
//   score (section 21), screen (section 23), pca (gv_pca_dev, section 24), king (gv_king_pairs, section 25).
// Every mode is "load data, maybe run vamp::infere, one or more data::Ax, a reduction, a file": the matvecs are HIP
// kernels behind libgvamp, the rest is host code.  One process per GPU (RANK / WORLD_SIZE from the launcher).
#include <algorithm>
#include <cmath>
#include <fstream>
#include <iostream>
#include <limits>
#include <sstream>

#include "data.hpp"
#include "options.hpp"
#include "score_cols.hpp"
#include "utilities.hpp"
#include "vamp.hpp"

namespace {

std::vector<double> load_estimate(const std::string& file, int M, int S) {
    // ".bin" = raw doubles at offset S*8 (mpi_read_vec_from_file), anything else = text, one value per line
    const size_t dot = file.find(".");
    const std::string ext = dot == std::string::npos ? "" : file.substr(dot + 1);
    std::vector<double> x = (ext == "bin") ? mpi_read_vec_from_file(file, M, S) : read_vec_from_file(file, M, S);
    x.resize(M, 0.0);
    return x;
}

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

}  // namespace

int main(int argc, char** argv) {
    const Options opt(argc, argv);
    const int rank = gv_env_rank();
    const std::string mode = opt.get_run_mode();
    const std::string type_data = opt.get_geno_format();      // [ext] --geno-format: "bed", or "dosage8" / "dosage16" code matrices
    const double dscale = opt.get_dosage_scale();
    const int dmiss = opt.get_dosage_missing();               // [ext] --dosage-missing: the all-ones code is a missing entry
    if (dmiss && type_data == "bed" && rank == 0)
        std::cout << "WARNING: --dosage-missing is ignored for --geno-format bed (PLINK rows carry their own missing code)" << std::endl;
    const int droute = opt.get_dosage_kernels() == "mfma" ? 1 : 0;      // [ext] --dosage-kernels: the route of the dosage products
    if (droute && type_data == "bed" && rank == 0)
        std::cout << "WARNING: --dosage-kernels is ignored for --geno-format bed (gv_set_kernel_mode selects the bed kernels)" << std::endl;
    const double alpha_scale = opt.get_alpha_scale();
    const std::string bimfp = opt.get_bim_file();
    const int dev = opt.get_device(), km = opt.get_kernel_mode();
    auto need_phen = [&](const std::vector<std::string>& files, const char* flag) {
        if (files.empty()) {
            std::cout << "FATAL  : no phen file(s) provided! Please use the " << flag << " option." << std::endl;
            exit(EXIT_FAILURE);
        }
    };

    // [ext] --ld-dosage 1 with --cg-precond ld: the data object's context accepts the LD preconditioner on 8-bit codes (DESIGN.md
    // section 18).  Without the flag vamp::infere's refusal stands.
    const bool pcd = opt.get_ld_dosage() == 1 && opt.get_cg_precond() == "ld" && type_data != "bed";
    if (pcd && (mode == "infere" || mode == "restart" || mode == "both") && type_data != "dosage8") {
        std::cout << "FATAL: --cg-precond ld with --ld-dosage 1 covers --geno-format dosage8 only, not --geno-format " << type_data << std::endl;
        return EXIT_FAILURE;
    }
    auto opt_in_ld_dosage = [&](data& ds) {
        if (pcd && gv_set_ld_dosage(ds.get_ctx(), 1)) {
            std::cout << "FATAL: gv_set_ld_dosage: " << gv_last_error(ds.get_ctx()) << std::endl;
            exit(EXIT_FAILURE);
        }
    };

    if (mode == "infere" || mode == "restart") {
        const int Mt = (int)opt.get_Mt(), N = (int)opt.get_N();
        std::vector<double> MS = divide_work(Mt);
        const int M = (int)MS[0], S = (int)MS[1];
        need_phen(opt.get_phen_files(), "--phen-files");
        data dataset(opt.get_phen_files()[0], opt.get_bed_file(), N, M, Mt, S, rank, type_data, alpha_scale, bimfp, dev, km, dscale, dmiss, droute);
        // infere: gam1 = 1e-6, gamw from --h2 (:64-69); restart: both from --gam1-init / --gamw-init (:381-382), r1 is
        // reloaded from --estimate-file inside infere_linear (vamp.cpp:226-233)
        const double gam1 = (mode == "restart") ? opt.get_gam1_init() : 1e-6;
        const double gamw = (mode == "restart") ? opt.get_gamw_init() : initial_gamw(opt);
        vamp emvamp(M, gam1, gamw, std::vector<double>(M, 0.0), rank, opt);
        opt_in_ld_dosage(dataset);
        infere_or_exit(emvamp, &dataset);
    } else if (mode == "test") {
        const int N_test = (int)opt.get_N_test(), Mt_test = (int)opt.get_Mt_test();
        std::vector<double> MS = divide_work(Mt_test);
        const int M_test = (int)MS[0], S_test = (int)MS[1];
        need_phen(opt.get_phen_files_test(), "--phen-files-test");
        data dataset_test(opt.get_phen_files_test()[0], opt.get_bed_file_test(), N_test, M_test, Mt_test, S_test, rank,
                          type_data, alpha_scale, bimfp, dev, km, dscale, dmiss, droute);
        std::vector<double> y_test = dataset_test.get_phen();
        const std::string est = opt.get_estimate_file();
        const size_t dot = est.find("."), pos_it = est.rfind("it");
        const std::string ext = est.substr(dot + 1);
        const std::vector<int> range = opt.get_test_iter_range();
        if (rank == 0) std::cout << "iter range = [" << range[0] << ", " << range[1] << "]" << std::endl;
        if (range[0] != -1) {                                                          // :152-181
            double maxR2 = -1;
            int maxind = -1;
            for (int it = range[0]; it <= range[1]; it++) {
                const std::string f = est.substr(0, pos_it) + "it_" + std::to_string(it) + "." + ext;
                const double R2 = test_r2(dataset_test, load_estimate(f, M_test, S_test), N_test, y_test, nullptr);
                if (rank == 0) std::cout << R2 << ", ";
                if (R2 > maxR2) {
                    maxR2 = R2;
                    maxind = it;
                }
            }
            if (rank == 0)
                std::cout << std::endl << "max R2 = " << maxR2 << std::endl << std::endl << "max ind = " << maxind << std::endl;
        } else {                                                                       // :183-211
            if (rank == 0) std::cout << "est_file_name = " << est << std::endl;
            double err2 = 0;
            const double R2 = test_r2(dataset_test, load_estimate(est, M_test, S_test), N_test, y_test, &err2);
            const double sd = calc_stdev(y_test);
            if (rank == 0) {
                std::cout << "y stdev^2 = " << sd * sd << std::endl;
                std::cout << "test l2 pred err^2 = " << err2 << std::endl;
                std::cout << "test R2 = " << R2 << std::endl;
            }
        }
    } else if (mode == "both") {                                                       // :214-283
        const int Mt = (int)opt.get_Mt(), N = (int)opt.get_N();
        std::vector<double> MS = divide_work(Mt);
        const int M = (int)MS[0], S = (int)MS[1];
        need_phen(opt.get_phen_files(), "--phen-files");
        need_phen(opt.get_phen_files_test(), "--phen-files-test");
        std::vector<double> x_est;
        double intercept, scale;
        {
            data dataset(opt.get_phen_files()[0], opt.get_bed_file(), N, M, Mt, S, rank, type_data, alpha_scale, bimfp, dev, km, dscale, dmiss, droute);
            vamp emvamp(M, 1e-6, initial_gamw(opt), std::vector<double>(M, 0.0), rank, opt);
            opt_in_ld_dosage(dataset);
            x_est = infere_or_exit(emvamp, &dataset);
            intercept = dataset.get_intercept();
            scale = dataset.get_scale();
        }
        if (rank == 0) std::cout << "intercept = " << intercept << std::endl << "scale = " << scale << std::endl;
        const int N_test = (int)opt.get_N_test(), Mt_test = (int)opt.get_Mt_test();
        data dataset_test(opt.get_phen_files_test()[0], opt.get_bed_file_test(), N_test, M, Mt_test, S, rank, type_data,
                          alpha_scale, bimfp, dev, km, dscale, dmiss, droute);
        std::vector<double> y_test = dataset_test.get_phen();
        double err2 = 0;
        const double R2 = test_r2(dataset_test, x_est, N_test, y_test, &err2, intercept, scale);   // :262-272
        const double sd = calc_stdev(y_test);
        if (rank == 0) {
            std::cout << std::endl << "y stdev^2 = " << sd * sd << std::endl;
            std::cout << "test l2 pred err^2 = " << err2 << std::endl;
            std::cout << "test R2 = " << R2 << std::endl;
        }
    } else if (mode == "pvals-calc") {                                                 // :284-368
        const int Mt = (int)opt.get_Mt(), N = (int)opt.get_N();
        std::vector<double> MS = divide_work(Mt);
        const int M = (int)MS[0], S = (int)MS[1];
        need_phen(opt.get_phen_files(), "--phen-files");
        data dataset(opt.get_phen_files()[0], opt.get_bed_file(), N, M, Mt, S, rank, type_data, alpha_scale, bimfp, dev, km, dscale, dmiss, droute);
        const std::string est = opt.get_estimate_file();
        const size_t dot = est.rfind("."), pos_it = est.rfind("it");
        const std::string ext = est.substr(dot + 1);
        const std::vector<int> range = opt.get_test_iter_range();
        if (rank == 0) std::cout << "iter range = [" << range[0] << ", " << range[1] << "]" << std::endl;
        std::vector<std::vector<double>> z1_hats, x1_hats;
        std::vector<std::string> out_loo, out_loco;
        const std::string pre = opt.get_out_dir() + opt.get_out_name();
        auto add = [&](const std::string& file, const std::string& tag) {
            std::vector<double> x = load_estimate(file, M, S);
            for (double& v : x) v *= sqrt((double)N);
            z1_hats.push_back(dataset.Ax(x.data()));
            x1_hats.push_back(x);
            out_loo.push_back(pre + tag + "_pvals.bin");
            out_loco.push_back(pre + tag);          // pvals_calc_LOCO appends "_pvals_LOCO.bin" (data.cpp:1347-1350)
        };
        if (range[0] != -1)
            for (int it = range[0]; it <= range[1]; it++)
                add(est.substr(0, pos_it) + "it_" + std::to_string(it) + "." + ext, "_it_" + std::to_string(it));
        else
            add(est, "");
        std::vector<double> y = dataset.filter_pheno();
        const int sp = (int)opt.get_store_pvals();   // 0 = LOO and LOCO, 1 = only LOO, 2 = only LOCO (:313)
        if (sp == 0 || sp == 1) dataset.pvals_calc(z1_hats, y, x1_hats, out_loo);
        if (dataset.get_bimfp() != "" && (sp == 0 || sp == 2)) dataset.pvals_calc_LOCO(z1_hats, y, x1_hats, out_loco);
    } else if (mode == "ldscore") {                                                    // [ext] DESIGN.md section 16
        // LD scores of the markers over --ld-window markers on each side, among the individuals with a phenotype
        const bool ldd = type_data == "dosage8" && opt.get_ld_dosage() == 1;      // [ext] --ld-dosage 1: DESIGN.md section 17
        if (type_data != "bed" && !ldd) {
            std::cout << "FATAL: --run-mode ldscore works on 2-bit genotypes only, not on --geno-format " << type_data << std::endl;
            return EXIT_FAILURE;
        }
        if (gv_env_nranks() > 1) {
            std::cout << "FATAL: --run-mode ldscore runs on one rank: the band stops at a shard's edges, so the scores of a sharded job "
                         "would miss their neighbours across them" << std::endl;
            return EXIT_FAILURE;
        }
        // [ext] DESIGN.md section 19: the window by distance (--ld-wind-kb / --ld-wind-cm) and the annotation categories (--ld-annot)
        const bool by_kb = opt.get_ld_wind_kb() >= 0, by_cm = opt.get_ld_wind_cm() >= 0, positional = by_kb || by_cm || opt.get_ld_annot() != "";
        if (opt.count_ld_windows() > 1) {
            std::cout << "FATAL: exactly one of --ld-window, --ld-wind-kb and --ld-wind-cm may be given" << std::endl;
            return EXIT_FAILURE;
        }
        if ((by_kb || by_cm) && bimfp == "") {
            std::cout << "FATAL: " << (by_kb ? "--ld-wind-kb" : "--ld-wind-cm") << " needs --bim-file: the positions are its "
                      << (by_kb ? "base-pair" : "cM") << " column" << std::endl;
            return EXIT_FAILURE;
        }
        const int Mt = (int)opt.get_Mt(), N = (int)opt.get_N();
        need_phen(opt.get_phen_files(), "--phen-files");
        data dataset(opt.get_phen_files()[0], opt.get_bed_file(), N, Mt, Mt, 0, rank, type_data, alpha_scale, bimfp, dev, km, dscale, dmiss, droute);
        if (ldd && gv_set_ld_dosage(dataset.get_ctx(), 1)) {
            std::cout << "FATAL: gv_set_ld_dosage: " << gv_last_error(dataset.get_ctx()) << std::endl;
            return EXIT_FAILURE;
        }
        const std::string pre = opt.get_out_dir() + opt.get_out_name();
        gv_ld_stats st;
        if (!positional) {
            const std::vector<std::vector<double>> res = dataset.ld_scores_dev(opt.get_ld_window(), opt.get_ld_adjust() == 1);
            gv_ld_info(dataset.get_ctx(), &st);
            mpi_store_vec_to_file(pre + "_ldscore.bin", res[0], 0, Mt);
            mpi_store_vec_to_file(pre + "_ldscore_n.bin", res[1], 0, Mt);
            std::cout << "LD scores: window " << opt.get_ld_window() << (opt.get_ld_adjust() ? " (adjusted)" : "") << ", " << Mt << " markers, "
                      << st.seconds << " seconds" << std::endl;
        } else {
            // the positions and the radius: kb of the base-pair column, cM of the cM column, or (an annotation with --ld-window) the indices
            std::vector<double> pos;
            double radius = (double)opt.get_ld_window();
            if (by_kb) {
                pos = dataset.read_positions(bimfp, "bp");
                radius = 1000.0 * opt.get_ld_wind_kb();
            } else if (by_cm) {
                pos = dataset.read_positions(bimfp, "cm");
                radius = opt.get_ld_wind_cm();
            } else
                for (int j = 0; j < Mt; j++) pos.push_back((double)j);
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
                if (!fm.good() || !fc.good()) {
                    std::cout << "FATAL: cannot write " << pre << "_ldscore_M.txt / _ldscore_cats.txt" << std::endl;
                    return EXIT_FAILURE;
                }
            }
            std::cout << "LD scores: window ";
            if (by_kb) std::cout << opt.get_ld_wind_kb() << " kb";
            else if (by_cm) std::cout << opt.get_ld_wind_cm() << " cM";
            else std::cout << opt.get_ld_window();
            std::cout << (opt.get_ld_adjust() ? " (adjusted)" : "") << ", " << Mt << " markers, " << C << (C == 1 ? " category, " : " categories, ")
                      << st.seconds << " seconds" << std::endl;
        }
    } else if (mode == "clump") {                                                      // [ext] DESIGN.md section 20
        // LD clumping of association results: the markers of p <= --clump-p1 in ascending p become index markers unless an earlier one
        // has claimed them; an index marker claims the markers of p <= --clump-p2 in its window with r^2 >= --clump-r2
        if (type_data != "bed") {
            std::cout << "FATAL: --run-mode clump works on 2-bit genotypes only, not on --geno-format " << type_data << std::endl;
            return EXIT_FAILURE;
        }
        if (gv_env_nranks() > 1) {
            std::cout << "FATAL: --run-mode clump runs on one rank: the band stops at a shard's edges, so the clumps of a sharded job "
                         "would miss their members across them" << std::endl;
            return EXIT_FAILURE;
        }
        const bool given_kb = opt.get_clump_kb() >= 0 || opt.get_ld_wind_kb() >= 0, by_cm = opt.get_ld_wind_cm() >= 0;
        const int windows = opt.count_ld_windows() + (opt.get_clump_kb() >= 0 ? 1 : 0);
        if (windows > 1) {
            std::cout << "FATAL: exactly one of --clump-kb, --ld-wind-cm and --ld-window may be given" << std::endl;
            return EXIT_FAILURE;
        }
        const bool by_kb = given_kb || windows == 0;            // (no window given: --clump-kb 250)
        const double kb = opt.get_clump_kb() >= 0 ? opt.get_clump_kb() : (opt.get_ld_wind_kb() >= 0 ? opt.get_ld_wind_kb() : 250.0);
        if ((by_kb || by_cm) && bimfp == "") {
            std::cout << "FATAL: " << (by_kb ? "--clump-kb" : "--ld-wind-cm") << " needs --bim-file: the positions are its "
                      << (by_kb ? "base-pair" : "cM") << " column" << std::endl;
            return EXIT_FAILURE;
        }
        const int Mt = (int)opt.get_Mt(), N = (int)opt.get_N();
        const std::string pfile = opt.get_clump_p_file();
        if (pfile == "") {
            std::cout << "FATAL: --run-mode clump needs --clump-p-file: " << Mt << " raw float64 p-values, the format of <out>_assoc_p.bin" << std::endl;
            return EXIT_FAILURE;
        }
        std::vector<double> p((size_t)Mt, 0.0);
        {
            std::ifstream fp(pfile, std::ios::binary | std::ios::ate);
            if (!fp.is_open()) {
                std::cout << "FATAL: cannot open the p file " << pfile << std::endl;
                return EXIT_FAILURE;
            }
            const long long bytes = (long long)fp.tellg();
            if (bytes < 8LL * Mt) {
                std::cout << "FATAL: the p file " << pfile << " holds " << bytes << " bytes, fewer than the " << 8LL * Mt << " of " << Mt
                          << " float64 values" << std::endl;
                return EXIT_FAILURE;
            }
            fp.seekg(0);
            fp.read(reinterpret_cast<char*>(p.data()), 8LL * Mt);
        }
        need_phen(opt.get_phen_files(), "--phen-files");
        data dataset(opt.get_phen_files()[0], opt.get_bed_file(), N, Mt, Mt, 0, rank, type_data, alpha_scale, bimfp, dev, km, dscale, dmiss, droute);
        std::vector<double> pos;
        double radius = (double)opt.get_ld_window();
        if (by_kb) {
            pos = dataset.read_positions(bimfp, "bp");
            radius = 1000.0 * kb;
        } else if (by_cm) {
            pos = dataset.read_positions(bimfp, "cm");
            radius = opt.get_ld_wind_cm();
        } else
            for (int j = 0; j < Mt; j++) pos.push_back((double)j);
        // the marker ids and chromosomes of the report: columns 2 and 1 of the .bim file, or m<j> and 0 without one
        std::vector<std::string> ids, chr;
        if (bimfp != "") {
            std::ifstream fb(bimfp);
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
        const std::string pre = opt.get_out_dir() + opt.get_out_name();
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
        if (!fc.good()) {
            std::cout << "FATAL: cannot write " << pre << "_clumps.txt" << std::endl;
            return EXIT_FAILURE;
        }
        std::cout << "LD clumping: window ";
        if (by_kb) std::cout << kb << " kb";
        else if (by_cm) std::cout << opt.get_ld_wind_cm() << " cM";
        else std::cout << opt.get_ld_window();
        std::cout << ", p1 " << opt.get_clump_p1() << ", p2 " << opt.get_clump_p2() << ", r2 " << opt.get_clump_r2() << ", " << Mt << " markers, "
                  << st.seconds << " seconds, " << n_index << " clumps, " << rounds << " rounds, " << st.block_pairs << " blocks launched"
                  << std::endl;
    } else if (mode == "score") {                                                      // [ext] DESIGN.md section 21
        // many weight vectors applied to a cohort in one go: <out>_scores.bin = C columns of N float64
        const int N_test = (int)opt.get_N_test(), Mt_test = (int)opt.get_Mt_test();
        const long long C0 = (long long)opt.get_score_cols();
        const std::string sfile = opt.get_score_file(), units = opt.get_score_units();
        const std::vector<double>& thr = opt.get_score_p_thresholds();
        const bool ct = !thr.empty() || opt.get_score_clump_index() != "" || opt.get_score_p_file() != "";
        if (sfile == "") {
            std::cout << "FATAL: --run-mode score needs --score-file: --score-cols x " << Mt_test << " raw float64 weights, column after column"
                      << std::endl;
            return EXIT_FAILURE;
        }
        if (ct && (thr.empty() || opt.get_score_clump_index() == "" || opt.get_score_p_file() == "")) {
            std::cout << "FATAL: --score-clump-index, --score-p-file and --score-p-thresholds go together: all three or none" << std::endl;
            return EXIT_FAILURE;
        }
        if (ct && C0 != 1) {
            std::cout << "FATAL: --score-p-thresholds builds its columns from column 0 of the score file: it needs --score-cols 1, not "
                      << C0 << std::endl;
            return EXIT_FAILURE;
        }
        // a whole file of `count` float64 values, FATAL with both byte counts when it is short
        auto read_f64 = [&](const std::string& file, const char* what, long long count, std::vector<double>& dst) {
            std::ifstream fp(file, std::ios::binary | std::ios::ate);
            if (!fp.is_open()) {
                std::cout << "FATAL: cannot open the " << what << " file " << file << std::endl;
                return false;
            }
            const long long bytes = (long long)fp.tellg();
            if (bytes < 8LL * count) {
                std::cout << "FATAL: the " << what << " file " << file << " holds " << bytes << " bytes, fewer than the " << 8LL * count
                          << " of " << count << " float64 values" << std::endl;
                return false;
            }
            dst.assign((size_t)count, 0.0);
            fp.seekg(0);
            fp.read(reinterpret_cast<char*>(dst.data()), 8LL * count);
            return true;
        };
        std::vector<double> wall, pall, iall;
        if (!read_f64(sfile, "score", C0 * Mt_test, wall)) return EXIT_FAILURE;
        if (ct && (!read_f64(opt.get_score_p_file(), "p", Mt_test, pall) || !read_f64(opt.get_score_clump_index(), "clump index", Mt_test, iall)))
            return EXIT_FAILURE;
        std::vector<double> MS = divide_work(Mt_test);
        const int M_test = (int)MS[0], S_test = (int)MS[1];
        data dataset_test(std::vector<double>(N_test, 0.0), opt.get_bed_file_test(), N_test, M_test, Mt_test, S_test, rank,
                          type_data, alpha_scale, bimfp, dev, km, dscale, dmiss, droute);
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
        if (units == "allele" && gv_env_nranks() > 1 && gv_allreduce_host(dataset_test.get_ctx(), konst.data(), (int)C)) {
            std::cout << "FATAL: gv_allreduce_host: " << gv_last_error(dataset_test.get_ctx()) << std::endl;
            return EXIT_FAILURE;
        }
        std::vector<std::vector<double>> z = dataset_test.score(cols);
        gv_score_stats st;
        gv_score_info(dataset_test.get_ctx(), &st);
        const std::string pre = opt.get_out_dir() + opt.get_out_name();
        if (rank == 0) {
            std::ofstream fo(pre + "_scores.bin", std::ios::binary);
            for (size_t k = 0; k < C; k++) {
                if (units == "allele")
                    for (int i = 0; i < N_test; i++) z[k][(size_t)i] += konst[k];
                fo.write(reinterpret_cast<const char*>(z[k].data()), 8LL * N_test);
            }
            fo.close();
            if (!fo.good()) {
                std::cout << "FATAL: cannot write " << pre << "_scores.bin" << std::endl;
                return EXIT_FAILURE;
            }
            std::cout << "scores: " << C << " columns (" << units << " units) x " << N_test << " individuals, "
                      << (st.path == GV_SCORE_PATH_KERNEL ? "kernel" : "fallback") << " path, " << st.passes << " passes, " << st.seconds
                      << " seconds -> " << pre << "_scores.bin" << std::endl;
        }
    } else if (mode == "screen") {                                                     // [ext] DESIGN.md section 23
        // every phenotype file against every marker: <out>_screen_{r,t,p}.bin = C columns of Mt float64
        if (type_data != "bed") {
            std::cout << "FATAL: --run-mode screen works on 2-bit genotypes only, not on --geno-format " << type_data << std::endl;
            return EXIT_FAILURE;
        }
        const int Mt = (int)opt.get_Mt(), N = (int)opt.get_N();
        std::vector<double> MS = divide_work(Mt);
        const int M = (int)MS[0], S = (int)MS[1];
        need_phen(opt.get_phen_files(), "--phen-files");
        const std::vector<std::string>& files = opt.get_phen_files();
        const size_t C = files.size();
        if ((long long)C * Mt > 2147483647LL) {
            std::cout << "FATAL: --run-mode screen: " << C << " columns x " << Mt << " markers exceed the 2^31 - 1 values of an output file" << std::endl;
            return EXIT_FAILURE;
        }
        // the third token of every line, NA -> NaN; complete cases: an individual with NA in any file is masked
        std::vector<std::vector<double>> Y(C);
        const size_t mb = (size_t)(N + 3) / 4;
        std::vector<unsigned char> m4(mb, 0);
        std::vector<char> have((size_t)N, 1);
        for (size_t c = 0; c < C; c++) {
            std::ifstream in(files[c]);
            if (!in.is_open()) {
                std::cout << "FATAL: could not open phenotype file: " << files[c] << std::endl;
                return EXIT_FAILURE;
            }
            std::string line;
            while (getline(in, line)) {
                std::istringstream ls(line);
                std::string a, b, v;
                if (!(ls >> a >> b >> v)) {
                    std::cout << "FATAL: phenotype line with fewer than 3 columns in " << files[c] << std::endl;
                    return EXIT_FAILURE;
                }
                Y[c].push_back(v == "NA" ? std::numeric_limits<double>::quiet_NaN() : atof(v.c_str()));
            }
            if ((int)Y[c].size() != N) {
                std::cout << "FATAL: " << files[c] << " holds " << Y[c].size() << " lines, not --N = " << N << std::endl;
                return EXIT_FAILURE;
            }
            for (int n = 0; n < N; n++)
                if (std::isnan(Y[c][(size_t)n])) have[(size_t)n] = 0;
        }
        int nonas = 0;
        for (int n = 0; n < N; n++)
            if (have[(size_t)n]) {
                m4[(size_t)n / 4] |= (unsigned char)(1u << (n % 4));
                nonas++;
            }
        if (nonas < 3) {
            std::cout << "FATAL: --run-mode screen: " << nonas << " complete cases leave the test no degree of freedom" << std::endl;
            return EXIT_FAILURE;
        }
        data dataset(std::vector<double>(N, 0.0), opt.get_bed_file(), N, M, Mt, S, rank, type_data, alpha_scale, bimfp, dev, km, dscale, dmiss,
                     droute);
        // [ext] --cov-file F --C K: the screen adjusted for K covariates and an intercept; complete cases over
        // the phenotype files and the covariates
        const bool with_cov = opt.get_cov_file() != "";
        const int K = with_cov ? (int)opt.get_C() : 0;
        if (with_cov) {
            if (K < 1 || K > GV_PCA_MAX_BLOCK) {
                std::cout << "FATAL: --run-mode screen --cov-file needs --C K, the number of covariates per line (1.." << GV_PCA_MAX_BLOCK << ")"
                          << std::endl;
                return EXIT_FAILURE;
            }
            dataset.read_covariates(opt.get_cov_file(), K);
            const std::vector<std::vector<double>> Z = dataset.get_covs();
            for (int n = 0; n < N; n++) {
                bool fin = true;
                for (int k = 0; k < K; k++) fin = fin && std::isfinite(Z[(size_t)n][(size_t)k]);
                if (!fin && have[(size_t)n]) {
                    have[(size_t)n] = 0;
                    m4[(size_t)n / 4] &= (unsigned char)~(1u << (n % 4));
                    nonas--;
                }
            }
            if (nonas - 2 - K < 1) {
                std::cout << "FATAL: --run-mode screen: " << nonas << " complete cases and " << K << " covariates leave the test no degree of freedom"
                          << std::endl;
                return EXIT_FAILURE;
            }
        }
        dataset.set_mask(m4, nonas);
        const std::string pre = opt.get_out_dir() + opt.get_out_name();
        if (with_cov) {
            const char* tag5[5] = {"_screen_r.bin", "_screen_t.bin", "_screen_p.bin", "_screen_beta.bin", "_screen_se.bin"};
            const size_t per5 = opt.get_screen_cols();
            dataset.screen_cov_set();
            gv_screen_cov_stats cs{};
            gv_screen_cov_info(dataset.get_ctx(), &cs);
            double prod = 0.0, panel = 0.0;
            for (size_t c0 = 0; c0 < C; c0 += per5) {
                const size_t c1 = c0 + per5 < C ? c0 + per5 : C;
                const std::vector<std::vector<double>> blk(Y.begin() + c0, Y.begin() + c1);
                const auto res = dataset.screen_cov(blk, opt.get_screen_vif());
                gv_screen_cov_info(dataset.get_ctx(), &cs);
                prod += cs.call_seconds_products;
                panel += cs.call_seconds_panel;
                for (int k = 0; k < 5; k++)
                    for (size_t c = c0; c < c1; c++) mpi_store_vec_to_file(pre + tag5[k], res[(size_t)k][c - c0], (int)(c * (size_t)Mt) + S, M);
            }
            if (rank == 0)
                std::cout << "screen: " << C << " phenotypes x " << Mt << " markers adjusted for " << K << " covariates, " << nonas
                          << " complete cases of " << N << ", nu = " << cs.nu << ", set " << cs.set_seconds << " seconds, products " << prod
                          << " s, panel and finishing kernels " << panel << " s -> " << pre << "_screen_{r,t,p,beta,se}.bin" << std::endl;
        }
        const char* tag[3] = {"_screen_r.bin", "_screen_t.bin", "_screen_p.bin"};
        const size_t per = opt.get_screen_cols();
        long long passes = 0;
        double seconds = 0.0;
        gv_atxm_stats st{};
        for (size_t c0 = 0; c0 < C && !with_cov; c0 += per) {
            const size_t c1 = c0 + per < C ? c0 + per : C;
            const std::vector<std::vector<double>> blk(Y.begin() + c0, Y.begin() + c1);
            const auto res = dataset.screen(blk);
            gv_atxm_info(dataset.get_ctx(), &st);
            passes += st.passes;
            seconds += st.seconds;
            for (int k = 0; k < 3; k++)
                for (size_t c = c0; c < c1; c++) mpi_store_vec_to_file(pre + tag[k], res[(size_t)k][c - c0], (int)(c * (size_t)Mt) + S, M);
        }
        if (rank == 0 && !with_cov)
            std::cout << "screen: " << C << " phenotypes x " << Mt << " markers, " << nonas << " complete cases of " << N << ", "
                      << (st.path == GV_ATXM_PATH_KERNEL ? "kernel" : "fallback") << " path, " << passes << " passes, " << seconds
                      << " seconds -> " << pre << "_screen_{r,t,p}.bin" << std::endl;
    } else if (mode == "pca") {                                                        // [ext] DESIGN.md section 24
        // the K leading principal components of the standardised genotypes among the individuals with a phenotype
        const int Mt = (int)opt.get_Mt(), N = (int)opt.get_N();
        const int K = (int)opt.get_pca_k();
        if (K < 1) {
            std::cout << "FATAL: --run-mode pca needs --pca-k K, the number of principal components (1.." << GV_PCA_MAX_BLOCK << ")" << std::endl;
            return EXIT_FAILURE;
        }
        const int L = opt.get_pca_block() ? (int)opt.get_pca_block() : std::min(GV_PCA_MAX_BLOCK, K + std::max(8, K));
        if (L < K || L > GV_PCA_MAX_BLOCK) {
            std::cout << "FATAL: --run-mode pca: the block has to hold --pca-k = " << K << " vectors and at most " << GV_PCA_MAX_BLOCK
                      << " (--pca-block " << L << ")" << std::endl;
            return EXIT_FAILURE;
        }
        if ((long long)K * Mt > 2147483647LL) {
            std::cout << "FATAL: --run-mode pca: " << K << " columns x " << Mt << " markers exceed the 2^31 - 1 values of an output file" << std::endl;
            return EXIT_FAILURE;
        }
        std::vector<double> MS = divide_work(Mt);
        const int M = (int)MS[0], S = (int)MS[1];
        need_phen(opt.get_phen_files(), "--phen-files");
        data dataset(opt.get_phen_files()[0], opt.get_bed_file(), N, M, Mt, S, rank, type_data, alpha_scale, bimfp, dev, km, dscale, dmiss, droute);
        const data::pca_result res = dataset.pca(K, L, opt.get_pca_tol(), (int)opt.get_pca_max_iter(), opt.get_pca_seed(), true);
        const std::string pre = opt.get_out_dir() + opt.get_out_name();
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
        if (rank == 0) {                                       // N-space is the same on every rank
            FILE* fv = fopen((pre + "_pca_eigenval.txt").c_str(), "w");
            FILE* fu = fopen((pre + "_pca_eigenvec.txt").c_str(), "w");
            bool ok = fv && fu;
            for (int i = 0; i < K && ok; i++) ok = fprintf(fv, "%.17g\n", res.eval[(size_t)i]) > 0;
            for (int n = 0; n < N && ok; n++)
                for (int i = 0; i < K && ok; i++) ok = fprintf(fu, i + 1 < K ? "%.17g " : "%.17g\n", res.evec[(size_t)i][(size_t)n]) > 0;
            if (fv) ok = fclose(fv) == 0 && ok;
            if (fu) ok = fclose(fu) == 0 && ok;
            if (!ok) {
                std::cout << "FATAL: cannot write " << pre << "_pca_eigenval.txt / _pca_eigenvec.txt" << std::endl;
                return EXIT_FAILURE;
            }
            std::cout << "pca: " << K << " components of " << N << " individuals x " << Mt << " markers, block " << L << ", "
                      << res.info.iterations << " iterations, " << (res.info.converged ? "converged" : "NOT converged") << " (largest r / theta = "
                      << worst << ", tol " << opt.get_pca_tol() << "), products " << res.info.seconds_products << " s, panel kernels "
                      << res.info.seconds_panel << " s -> " << pre << "_pca_{eigenval.txt,eigenvec.txt,loadings.bin}" << std::endl;
        }
    } else if (mode == "king") {                                                       // [ext] DESIGN.md section 25
        // the pairs of individuals at or above a kinship cutoff, from the genotypes alone: no phenotype file
        if (type_data != "bed") {
            std::cout << "FATAL: --run-mode king works on 2-bit genotypes only, not on --geno-format " << type_data << std::endl;
            return EXIT_FAILURE;
        }
        if (gv_env_nranks() > 1) {
            std::cout << "FATAL: --run-mode king runs on one rank: the counts of a pair are sums over the markers of all ranks, and the "
                         "integer all-reduce that would add them is not built" << std::endl;
            return EXIT_FAILURE;
        }
        const int Mt = (int)opt.get_Mt(), N = (int)opt.get_N();
        std::vector<unsigned char> use;
        if (opt.get_king_marker_file() != "") {
            std::ifstream in(opt.get_king_marker_file(), std::ios::binary);
            use.assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
            if (!in.is_open() || use.size() != (size_t)Mt) {
                std::cout << "FATAL: --king-marker-file " << opt.get_king_marker_file() << " must hold Mt = " << Mt << " bytes of 0 / 1 ("
                          << (in.is_open() ? std::to_string(use.size()) + " bytes read" : std::string("cannot open it")) << ")" << std::endl;
                return EXIT_FAILURE;
            }
        }
        setenv("GVAMP_RESIDENT_LAYOUT", "2", 0);      // the kernel reads the tile layout (a --resident-layout given on the command line stands)
        data dataset(std::vector<double>(N, 0.0), opt.get_bed_file(), N, Mt, Mt, 0, rank, type_data, alpha_scale, bimfp, dev, km);
        const data::king_result res = dataset.king_pairs(opt.get_king_cutoff(), use);
        const std::string path = opt.get_out_dir() + opt.get_out_name() + "_king.kin0.txt";
        FILE* f = fopen(path.c_str(), "w");
        bool ok = f != nullptr;
        for (size_t t = 0; t < res.i.size() && ok; t++) {
            const int32_t* q = &res.counts[5 * t];
            ok = fprintf(f, "%d %d %d %d %d %d %d %.17g\n", res.i[t], res.j[t], q[0], q[1], q[2], q[3], q[4], res.kin[t]) > 0;
        }
        if (f) ok = fclose(f) == 0 && ok;
        if (!ok) {
            std::cout << "FATAL: cannot write " << path << std::endl;
            return EXIT_FAILURE;
        }
        std::cout << "king: " << N << " individuals x " << res.info.used_markers << " of " << Mt << " markers, cutoff " << opt.get_king_cutoff()
                  << ": " << res.i.size() << " pairs, " << res.info.seconds << " seconds -> " << path << std::endl;
    } else if (mode == "predict" || mode == "predict_single") {                        // :386-594
        const int N_test = (int)opt.get_N_test(), Mt_test = (int)opt.get_Mt_test();
        std::vector<double> MS = divide_work(Mt_test);
        const int M_test = (int)MS[0], S_test = (int)MS[1];
        data dataset_test(std::vector<double>(N_test, 0.0), opt.get_bed_file_test(), N_test, M_test, Mt_test, S_test, rank,
                          type_data, alpha_scale, bimfp, dev, km, dscale, dmiss, droute);
        const std::string est = opt.get_estimate_file();
        const std::string ext = est.substr(est.find(".") + 1);
        const std::string pre = opt.get_out_dir() + opt.get_out_name();
        auto predict = [&](const std::string& file) {
            std::vector<double> x = load_estimate(file, M_test, S_test);
            for (double& v : x) v *= sqrt((double)N_test);
            return dataset_test.Ax(x.data());
        };
        if (mode == "predict_single") {
            std::vector<double> z = predict(est);
            if (rank == 0) {
                std::cout << "filepath_out = " << pre + "_predict.csv" << std::endl;
                store_vec_to_file(pre + "_predict.csv", z);
            }
        } else {
            if (rank == 0) std::cout << "est_file_name = " << est << std::endl;
            const size_t pos_it = est.rfind("temp");
            const std::vector<int> range = opt.get_test_iter_range();
            if (rank == 0) std::cout << "iter range = [" << range[0] << ", " << range[1] << "]" << std::endl;
            if (range[0] != -1) {
                std::vector<std::vector<double>> zs;
                for (int it = range[0]; it <= range[1]; it++) {
                    const std::string f = est.substr(0, pos_it) + "temp_" + std::to_string(it) + "_" + std::to_string(it) +
                                          "_gibbs_est." + ext;
                    if (rank == 0) std::cout << "est_file_name_it = " << f << std::endl;
                    zs.push_back(predict(f));
                }
                for (int i = 0; i < N_test && rank == 0; i++) {       // one csv per individual (:424-434)
                    std::vector<double> row;
                    for (auto& z : zs) row.push_back(z[i]);
                    store_vec_to_file(pre + "_predict_" + std::to_string(i) + ".csv", row);
                }
            }
        }
    } else {
        std::cout << "FATAL: unknown --run-mode \"" << mode << "\"" << std::endl;
        return EXIT_FAILURE;
    }
    gv_host_finalize();      // the process's communicator, after the last data object (MPI_Finalize of the reference)
    return 0;
}
