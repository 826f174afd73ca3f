// options.cpp -- table-driven parser for the reference's command line (options.cpp:18-429).
#include "options.hpp"

#include <sys/stat.h>

#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <map>
#include <sstream>

namespace {
int rank_for_printing() {
    const char* r = getenv("RANK");
    return r ? atoi(r) : 0;
}
[[noreturn]] void fatal(const std::string& msg) {
    std::cout << msg << std::endl;
    exit(EXIT_FAILURE);
}
std::vector<std::string> split_commas(const std::string& s) {
    std::vector<std::string> out;
    std::stringstream ss(s);
    std::string item;
    while (getline(ss, item, ',')) out.push_back(item);
    return out;
}
void existing_files(const std::string& cslist, std::vector<std::string>& dst) {   // options.cpp:73-123
    for (const std::string& fp : split_commas(cslist)) {
        std::ifstream f(fp);
        if (!f.is_open()) fatal("FATAL: file " + fp + " not found");
        dst.push_back(fp);
    }
}
enum Check { ANY, NONNEG, POS };
unsigned int checked_uint(const char* flag, const char* arg, Check chk, const char* what) {
    int v = atoi(arg);
    if ((chk == NONNEG && v < 0) || (chk == POS && v < 1))
        fatal(std::string("FATAL  : option ") + flag + " has to be " + what + "! (" + arg + " was passed)");
    return (unsigned int)v;
}
}  // namespace

void Options::fail_if_last(char** argv, const int i) {
    std::cout << "FATAL  : missing argument for last option \"" << argv[i]
              << "\". Please check your input and relaunch." << std::endl;
    exit(EXIT_FAILURE);
}

void Options::read_command_line_options(int argc, char** argv) {
    using Handler = std::function<void(const char*)>;
    std::map<std::string, Handler> H;
    auto str = [&](const char* f, std::string& dst) { H[f] = [&dst](const char* a) { dst = a; }; };
    auto dbl = [&](const char* f, double& dst) { H[f] = [&dst](const char* a) { dst = atof(a); }; };
    auto uns = [&](const char* f, unsigned int& dst, Check chk, const char* what) {
        std::string flag = f;
        H[f] = [&dst, chk, what, flag](const char* a) { dst = checked_uint(flag.c_str(), a, chk, what); };
    };
    str("--bed-file", bed_file);
    str("--cov-file", cov_file);
    str("--bed-file-test", bed_file_test);
    str("--estimate-file", estimate_file);
    str("--freeze-index-file", freeze_index_file);
    str("--cov-estimate-file", cov_estimate_file);
    str("--run-mode", run_mode);
    str("--out-name", out_name);
    str("--model", model);
    str("--bim-file", bim_file);
    H["--phen-files"] = [&](const char* a) { existing_files(a, phen_files); };
    H["--true-signal-files"] = [&](const char* a) { existing_files(a, true_signal_files); };
    H["--phen-files-test"] = [&](const char* a) { existing_files(a, phen_files_test); };
    H["--vars"] = [&](const char* a) { for (auto& v : split_commas(a)) vars.push_back(atof(v.c_str())); };
    H["--probs"] = [&](const char* a) { for (auto& v : split_commas(a)) probs.push_back(atof(v.c_str())); };
    H["--test-iter-range"] = [&](const char* a) {
        int nit = 0;
        for (auto& v : split_commas(a)) if (nit < 2) test_iter_range[nit++] = atoi(v.c_str());
    };
    H["--out-dir"] = [&](const char* a) {   // created on parse (options.cpp:271-279)
        out_dir = a;
        struct stat st;
        if (stat(a, &st) != 0) mkdir(a, 0777);
    };
    uns("--use-lmmse-damp", use_lmmse_damp, NONNEG, "a non-negative integer");
    uns("--use-freeze", use_freeze, NONNEG, "a non-negative integer");
    uns("--seed", seed, NONNEG, "a non-negative integer");
    uns("--learn-vars", learn_vars, NONNEG, "a non-negative integer");
    uns("--use-XXT-denoiser", use_XXT_denoiser, NONNEG, "a non-negative integer");
    uns("--iterations", iterations, POS, "a strictly positive integer");
    uns("--num-mix-comp", num_mix_comp, POS, "a strictly positive integer");
    uns("--store-pvals", store_pvals, NONNEG, "an integer");
    uns("--red", redglob, NONNEG, "an integer");
    uns("--init-est", init_est, NONNEG, "an integer");
    uns("--EM-max-iter", EM_max_iter, POS, "a strictly positive integer");
    uns("--Mt", Mt, POS, "a strictly positive integer");
    uns("--CV", CV, NONNEG, "a positive integer");
    uns("--C", C, NONNEG, "a non-negative integer");
    uns("--N", N, POS, "a strictly positive integer");
    uns("--N-test", N_test, POS, "a strictly positive integer");
    uns("--Mt-test", Mt_test, POS, "a strictly positive integer");
    uns("--CG-max-iter", CG_max_iter, POS, "a strictly positive integer");
    dbl("--stop-criteria-thr", stop_criteria_thr);
    dbl("--EM-err-thr", EM_err_thr);
    dbl("--alpha-scale", alpha_scale);
    dbl("--rho", rho);
    dbl("--gamma-damp", gamma_damp);
    dbl("--gam1-init", gam1_init);
    dbl("--gamw-init", gamw_init);
    dbl("--probit-var", probit_var);
    dbl("--h2", h2);
    // [ext]
    H["--device"] = [&](const char* a) { device = atoi(a); };
    H["--kernel-mode"] = [&](const char* a) { kernel_mode = atoi(a); };
    H["--synth-seed"] = [&](const char* a) { synth_seed = atol(a); };
    uns("--synth-miss-ppm", synth_miss_ppm, NONNEG, "a non-negative integer");
    H["--diagnostics"] = [&](const char* a) { diagnostics = atoi(a); };
    H["--store-iterates"] = [&](const char* a) { store_iterates = atoi(a); };
    H["--fuse-solves"] = [&](const char* a) { fuse_solves = atoi(a); };
    H["--reanchor-every"] = [&](const char* a) { reanchor_every = atoi(a) < 0 ? 0 : atoi(a); };
    H["--huber-delta-schedule"] = [&](const char* a) {
        if (strcmp(a, "deferred") && strcmp(a, "reference"))
            fatal(std::string("FATAL  : option --huber-delta-schedule has to be deferred or reference! (") + a + " was passed)");
        huber_delta_schedule = a;
    };
    H["--cg-precond"] = [&](const char* a) {
        if (strcmp(a, "scalar") && strcmp(a, "ld"))
            fatal(std::string("FATAL  : option --cg-precond has to be scalar or ld! (") + a + " was passed)");
        cg_precond = a;
    };
    H["--cg-precond-window"] = [&](const char* a) {
        if (strcmp(a, "32") && strcmp(a, "64") && strcmp(a, "128"))
            fatal(std::string("FATAL  : option --cg-precond-window has to be 32, 64 or 128! (") + a + " was passed)");
        cg_precond_window = atoi(a);
    };
    H["--geno-format"] = [&](const char* a) {
        if (strcmp(a, "bed") && strcmp(a, "dosage8") && strcmp(a, "dosage16"))
            fatal(std::string("FATAL  : option --geno-format has to be bed, dosage8 or dosage16! (") + a + " was passed)");
        geno_format = a;
    };
    H["--dosage-scale"] = [&](const char* a) {
        if (!(atof(a) > 0) || atof(a) > 1e300)
            fatal(std::string("FATAL  : option --dosage-scale has to be a positive number! (") + a + " was passed)");
        dosage_scale = atof(a);
    };
    H["--dosage-missing"] = [&](const char* a) {
        if (strcmp(a, "0") && strcmp(a, "1"))
            fatal(std::string("FATAL  : option --dosage-missing has to be 0 or 1! (") + a + " was passed)");
        dosage_missing = atoi(a);
    };
    H["--screen-dosage"] = [&](const char* a) {
        if (strcmp(a, "0") && strcmp(a, "1"))
            fatal(std::string("FATAL  : option --screen-dosage has to be 0 or 1! (") + a + " was passed)");
        screen_dosage = atoi(a);
    };
    H["--dosage-kernels"] = [&](const char* a) {
        if (strcmp(a, "valu") && strcmp(a, "mfma"))
            fatal(std::string("FATAL  : option --dosage-kernels has to be valu or mfma! (") + a + " was passed)");
        dosage_kernels = a;
    };
    H["--store-assoc"] = [&](const char* a) {
        if (strcmp(a, "0") && strcmp(a, "1"))
            fatal(std::string("FATAL  : option --store-assoc has to be 0 or 1! (") + a + " was passed)");
        store_assoc = (unsigned int)atoi(a);
    };
    H["--ld-window"] = [&](const char* a) {
        if (atoi(a) < 1 || atoi(a) > 8192)
            fatal(std::string("FATAL  : option --ld-window has to be within 1..8192! (") + a + " was passed)");
        ld_window = atoi(a);
        ld_windows_given++;
    };
    auto wind = [&](const char* f, double& dst) {
        std::string flag = f;
        H[f] = [&dst, flag, this](const char* a) {
            char* end = nullptr;
            const double v = strtod(a, &end);
            if (end == a || *end != 0 || !(v >= 0) || v > 1e300)
                fatal("FATAL  : option " + flag + " has to be a non-negative number! (" + a + " was passed)");
            dst = v;
            ld_windows_given++;
        };
    };
    wind("--ld-wind-kb", ld_wind_kb);
    wind("--ld-wind-cm", ld_wind_cm);
    str("--ld-annot", ld_annot);
    str("--clump-p-file", clump_p_file);
    auto num = [&](const char* f, double& dst) {          // a whole token as a number (NaN and infinities are the library's to refuse)
        std::string flag = f;
        H[f] = [&dst, flag](const char* a) {
            char* end = nullptr;
            const double v = strtod(a, &end);
            if (end == a || *end != 0) fatal("FATAL  : option " + flag + " has to be a number! (" + a + " was passed)");
            dst = v;
        };
    };
    num("--clump-p1", clump_p1);
    num("--clump-p2", clump_p2);
    num("--clump-r2", clump_r2);
    H["--clump-kb"] = [&](const char* a) {
        char* end = nullptr;
        const double v = strtod(a, &end);
        if (end == a || *end != 0 || !(v >= 0) || v > 1e300)
            fatal(std::string("FATAL  : option --clump-kb has to be a non-negative number! (") + a + " was passed)");
        clump_kb = v;
    };
    str("--score-file", score_file);
    str("--score-clump-index", score_clump_index);
    str("--score-p-file", score_p_file);
    uns("--score-cols", score_cols, POS, "a strictly positive integer");
    uns("--screen-cols", screen_cols, POS, "a strictly positive integer");
    num("--screen-vif", screen_vif);
    uns("--pca-k", pca_k, POS, "a strictly positive integer");
    uns("--pca-block", pca_block, POS, "a strictly positive integer");
    uns("--pca-max-iter", pca_max_iter, POS, "a strictly positive integer");
    uns("--pca-seed", pca_seed, NONNEG, "a non-negative integer");
    uns("--pca-allow-unconverged", pca_allow_unconverged, NONNEG, "a non-negative integer");
    num("--pca-tol", pca_tol);
    num("--king-cutoff", king_cutoff);
    str("--king-marker-file", king_marker_file);
    H["--grm-cutoff"] = [&](const char* a) {              // (given at all: the sparse file; NaN and +inf are the library's to refuse)
        char* end = nullptr;
        const double v = strtod(a, &end);
        if (end == a || *end != 0) fatal(std::string("FATAL  : option --grm-cutoff has to be a number! (") + a + " was passed)");
        grm_cutoff = v;
        grm_has_cutoff = 1;
    };
    str("--grm-marker-file", grm_marker_file);
    H["--score-units"] = [&](const char* a) {
        if (strcmp(a, "std") && strcmp(a, "allele"))
            fatal(std::string("FATAL  : option --score-units has to be std or allele! (") + a + " was passed)");
        score_units = a;
    };
    H["--score-p-thresholds"] = [&](const char* a) {
        score_p_thresholds.clear();
        for (auto& v : split_commas(a)) {
            char* end = nullptr;
            const double t = strtod(v.c_str(), &end);
            if (end == v.c_str() || *end != 0 || !(t >= 0))
                fatal(std::string("FATAL  : option --score-p-thresholds has to be a comma-separated list of non-negative numbers! (") + a +
                      " was passed)");
            score_p_thresholds.push_back(t);
        }
    };
    H["--ld-adjust"] = [&](const char* a) {
        if (strcmp(a, "0") && strcmp(a, "1"))
            fatal(std::string("FATAL  : option --ld-adjust has to be 0 or 1! (") + a + " was passed)");
        ld_adjust = atoi(a);
    };
    H["--ld-dosage"] = [&](const char* a) {
        if (strcmp(a, "0") && strcmp(a, "1"))
            fatal(std::string("FATAL  : option --ld-dosage has to be 0 or 1! (") + a + " was passed)");
        ld_dosage = atoi(a);
    };
    H["--resident-layout"] = [&](const char* a) {      // read by data::open_device (every data object of the run)
        resident_layout = atoi(a);
        setenv("GVAMP_RESIDENT_LAYOUT", a, 1);
    };

    std::stringstream ss;
    ss << "\nardyh command line options:\n";
    for (int i = 1; i < argc; ++i) {
        auto it = H.find(argv[i]);
        if (it == H.end()) {   // options.cpp:421-424
            std::cout << "FATAL: option \"" << argv[i] << "\" unknown\n";
            exit(EXIT_FAILURE);
        }
        if (i == argc - 1) fail_if_last(argv, i);
        const char* arg = argv[++i];
        it->second(arg);
        ss << argv[i - 1] << " " << arg << "\n";
    }
    if (rank_for_printing() == 0) std::cout << ss.str() << std::endl;
    // [ext] what --resident-layout 3 (auto) may assume about the length of the run: every data object of the process tells the
    // library to expect about 12 ATx passes per VAMP iteration (4-40 in the runs measured), gv_set_expected_passes -- below 1 000 passes a
    // second stripe set does not earn its allocation back and auto takes the one tile layout (as it does for a caller that says
    // nothing: bench.py and a bare binding get the same layout as a driver run of fewer than 84 iterations).  $GVAMP_EXPECTED_PASSES overrides.
    if (!getenv("GVAMP_EXPECTED_PASSES")) setenv("GVAMP_EXPECTED_PASSES", std::to_string((long long)iterations * 12).c_str(), 1);
}

void Options::list_phen_files() const {
    for (const auto& p : phen_files) std::cout << " phen file: " << p << std::endl;
}

void Options::check_options() {   // options.cpp:447-493: a bed file is the only hard requirement
    if (get_bed_file() == "" && get_bed_file_test() == "" && synth_seed < 0) {
        std::cout << "FATAL  : no bed file provided! Please use the --bed-file option." << std::endl;
        exit(EXIT_FAILURE);
    }
}
