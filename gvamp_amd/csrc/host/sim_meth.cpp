// sim_meth.cpp -- driver of a simulated methylation (EWAS) run, a restatement of the reference's main_meth_ex.cpp (which no longer
// compiles against its own `data` constructor): an i.i.d. N(0, 1) design matrix written to --bed-file at byte offset S*N*8 and read
// back as type_data == "meth"; prior {0.98, 0.02} / {0, 1e-3}; noise precision from SNR 2 (noise_prec_calc); y = A (beta sqrt(N)) +
// noise; vamp::infere from gamw_init = 0.9 gamw.  The reference seeds the noise from std::random_device; here it comes from --seed,
// as sim.cpp does, so that a run can be repeated.  One process per GPU; ranks from RANK / WORLD_SIZE.
// [ext] --synth-seed S generates the matrix on the device (gv_synth_meth) instead of writing and reading a file: EWAS-size runs stay
// off the disk.
#include <fcntl.h>
#include <unistd.h>

#include <cerrno>
#include <cmath>
#include <cstring>
#include <iostream>
#include <random>

#include "data.hpp"
#include "options.hpp"
#include "utilities.hpp"
#include "vamp.hpp"

// this rank's M x N doubles at byte offset S*N*8 of the file (64-bit offsets throughout)
static bool write_slice(const std::string& path, const std::vector<double>& v, size_t offset_bytes) {
    const int fd = open(path.c_str(), O_CREAT | O_WRONLY, 0644);
    if (fd < 0) return false;
    const char* p = reinterpret_cast<const char*>(v.data());
    size_t left = v.size() * sizeof(double), done = 0;
    while (left > 0) {
        const ssize_t w = pwrite(fd, p + done, left, (off_t)(offset_bytes + done));
        if (w < 0 && errno == EINTR) continue;
        if (w <= 0) { close(fd); return false; }
        done += (size_t)w;
        left -= (size_t)w;
    }
    return close(fd) == 0;
}

int main(int argc, char** argv) {
    const Options opt(argc, argv);
    const int rank = gv_env_rank(), nranks = gv_env_nranks();
    const size_t Mt = opt.get_Mt(), N = opt.get_N();
    std::vector<double> MS = divide_work((int)Mt);
    const int M = (int)MS[0], S = (int)MS[1];
    const long unsigned int seed = opt.get_seed();

    data* dataset;
    gv_ctx* synth_ctx = nullptr;
    if (opt.get_synth_seed() >= 0) {
        if (nranks > 1) {
            std::cout << "FATAL: --synth-seed with WORLD_SIZE > 1 is not supported by this driver" << std::endl;
            return EXIT_FAILURE;
        }
        int dev = opt.get_device() >= 0 ? opt.get_device() : gv_env_local_rank();
        if (gv_create(dev, &synth_ctx) || gv_set_dims(synth_ctx, N, M, Mt, S) ||
            gv_synth_meth(synth_ctx, (uint64_t)opt.get_synth_seed())) {
            std::cout << "FATAL: " << gv_last_error(synth_ctx) << std::endl;
            return EXIT_FAILURE;
        }
        dataset = new data(synth_ctx, std::vector<double>(N, 0.0), (int)N, M, (int)Mt, S, rank);
    } else {
        // main_meth_ex.cpp:38-41: simulate(N*M, {1}, {1}) -- element e of the global matrix draws with seed + e, so every rank
        // writes its own slice of one matrix
        const std::vector<double> one{1.0};
        std::vector<double> mat((size_t)M * N);
        const size_t e0 = (size_t)S * N;
        for (size_t e = 0; e < mat.size(); e++) mat[e] = simulate(1, one, one, seed + e0 + e)[0];
        if (!write_slice(opt.get_bed_file(), mat, e0 * sizeof(double))) {
            std::cout << "FATAL: could not write the methylation matrix to " << opt.get_bed_file() << std::endl;
            return EXIT_FAILURE;
        }
        mat.clear();
        mat.shrink_to_fit();
        dataset = new data(std::vector<double>(N, 0.0), opt.get_bed_file(), (int)N, M, (int)Mt, S, rank, "meth", 1.0, "",
                           opt.get_device(), opt.get_kernel_mode());
    }

    const std::vector<double> vars{0, 1e-3}, probs{0.98, 0.02};                   // main_meth_ex.cpp:58-63
    std::vector<double> vars_init = opt.get_vars(), probs_init = opt.get_probs();
    if (rank == 0) {
        std::cout << "true scaled variances = ";
        for (double v : vars) std::cout << v * N << ' ';
        std::cout << std::endl << "true probs = ";
        for (double p : probs) std::cout << p << ' ';
        std::cout << std::endl;
    }
    const double SNR = 2;
    const double gamw = noise_prec_calc(SNR, vars, probs, (int)Mt, (int)N);
    if (rank == 0) std::cout << "true gamw = " << gamw << std::endl;

    std::vector<double> beta_all = simulate((int)Mt, vars, probs, seed + 1);      // every rank draws the same beta
    std::vector<double> beta_true(M, 0.0);
    for (int i = 0; i < M; i++) beta_true[i] = beta_all[S + i];
    mpi_store_vec_to_file(opt.get_out_dir() + opt.get_out_name() + "_beta_true.bin", beta_true, S, M);
    std::mt19937 generator{seed};
    std::normal_distribution<double> gauss_beta_gen(0, 1 / sqrt(gamw));
    std::vector<double> noise(N, 0.0);
    for (size_t i = 0; i < N; i++) noise[i] = gauss_beta_gen(generator);
    if (rank == 0) std::cout << "noise prec = " << 1.0 / pow(calc_stdev(noise), 2) << std::endl;
    std::vector<double> beta_true_scaled = beta_true;
    for (double& b : beta_true_scaled) b *= sqrt((double)N);
    std::vector<double> y = dataset->Ax(beta_true_scaled.data());
    if (rank == 0) std::cout << "Var(Ax) = " << pow(calc_stdev(y), 2) << std::endl;
    y.resize(N);
    for (size_t i = 0; i < N; i++) y[i] += noise[i];
    dataset->set_phen(y);
    if (rank == 0) {
        store_vec_to_file(opt.get_out_dir() + opt.get_out_name() + "_y.txt", y);
        mpi_store_vec_to_file(opt.get_out_dir() + opt.get_out_name() + "_y.bin", y, 0, (int)N);   // [ext] y at full precision
        std::cout << "Var(y) = " << pow(calc_stdev(y), 2) << std::endl;
        const double r = calc_stdev(noise) / calc_stdev(y);
        std::cout << "true R2 = " << 1 - r * r << std::endl;
    }

    const double gamw_init = 0.9 * gamw, gam1 = 1e-6;                           // main_meth_ex.cpp:163-164
    {   // the vamp object owns device vectors of the dataset's context: it must go first
        vamp emvamp((int)N, M, (int)Mt, gam1, gamw_init, opt.get_iterations(), opt.get_rho(), vars_init, probs_init,
                    beta_true, rank, opt.get_out_dir(), opt.get_out_name(), opt.get_model(), opt);
        std::vector<double> x_est = infere_or_exit(emvamp, dataset);
    }
    if (rank == 0) {
        std::cout << "var(y) = " << pow(calc_stdev(y), 2) << std::endl;
        std::cout << "true gamw = " << gamw << std::endl;
        std::cout << "noise prec = " << 1.0 / pow(calc_stdev(noise), 2) << std::endl;
    }
    delete dataset;
    if (synth_ctx) gv_destroy(synth_ctx);
    gv_host_finalize();
    return 0;
}
