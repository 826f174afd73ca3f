// data.cpp -- see data.hpp.
#include "data.hpp"

#include <algorithm>
#include <cassert>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>
#include <sstream>
#include <sys/stat.h>
#include <ctime>

#include <unistd.h>

#include "shm_comm.hpp"
#include "utilities.hpp"

namespace {
[[noreturn]] void die(const std::string& msg) {
    std::cout << msg << std::endl;
    exit(EXIT_FAILURE);
}
void ck(gv_ctx* ctx, int rc, const char* what) {
    if (rc) die(std::string("FATAL: ") + what + ": " + gv_last_error(ctx));
}
// n device vectors of one space, freed with the object.  put(): a host column, cut or zero-padded to the vector's length (4 * mbytes
// in N-space, M in M-space); get(): the vector's values
struct dev_cols {
    gv_ctx* ctx;
    std::vector<gv_vec*> h;
    dev_cols(gv_ctx* ctx, int space, size_t n) : ctx(ctx), h(n, nullptr) {
        for (gv_vec*& v : h) ck(ctx, gv_vec_alloc(ctx, space, &v), "gv_vec_alloc");
    }
    ~dev_cols() {
        for (gv_vec* v : h) gv_vec_free(ctx, v);
    }
    dev_cols(const dev_cols&) = delete;
    dev_cols& operator=(const dev_cols&) = delete;
    void put(size_t i, std::vector<double> col) {
        col.resize((size_t)std::max<int64_t>(gv_vec_len(h[i]), 1), 0.0);
        ck(ctx, gv_vec_upload(ctx, h[i], col.data()), "gv_vec_upload");
    }
    std::vector<double> get(size_t i) const {
        std::vector<double> col((size_t)std::max<int64_t>(gv_vec_len(h[i]), 1), 0.0);
        ck(ctx, gv_vec_download(ctx, h[i], col.data()), "gv_vec_download");
        col.resize((size_t)std::max<int64_t>(gv_vec_len(h[i]), 0));
        return col;
    }
};
// whitespace split that keeps the reference's quirk: a leading blank yields an empty token 0 (std::regex
// "\\s+" with sregex_token_iterator(-1), data.cpp:143-144)
std::vector<std::string> split_ws(const std::string& line) {
    std::vector<std::string> tok;
    size_t i = 0, n = line.size();
    if (n && isspace((unsigned char)line[0])) {
        tok.push_back("");
        while (i < n && isspace((unsigned char)line[i])) i++;
    }
    while (i < n) {
        size_t j = i;
        while (j < n && !isspace((unsigned char)line[j])) j++;
        tok.push_back(line.substr(i, j - i));
        i = j;
        while (i < n && isspace((unsigned char)line[i])) i++;
    }
    return tok;
}
}  // namespace

namespace {
int dosage_bits(const std::string& type_data) { return type_data == "dosage8" ? 8 : (type_data == "dosage16" ? 16 : 0); }
void check_type_data(const std::string& type_data) {
    if (type_data != "bed" && type_data != "meth" && !dosage_bits(type_data))
        die("FATAL: type_data must be \"bed\", \"meth\", \"dosage8\" or \"dosage16\", not \"" + type_data + "\"");
}
}  // namespace

void data::open_device(int device, int kernel_mode) {
    if (device < 0) device = gv_env_local_rank();
    if (gv_env_nranks() > 1) (void)gv_bind_host_numa(device, nullptr);   // one process per GPU: stay on the CPUs next to it
    if (gv_create(device, &ctx)) die(std::string("FATAL: ") + gv_last_error(nullptr));
    ck(ctx, gv_set_dims(ctx, N, M, Mt, S), "gv_set_dims");
    // kernel mode 1: two stripe sets (1), the single tile layout (2: half the HBM, same bits), or -- the default, 3 -- the tile
    // layout unless the run is long (>= 1000 expected ATx passes) and two stripe sets fit the free HBM (--resident-layout)
    const char* lay = getenv("GVAMP_RESIDENT_LAYOUT");
    const int stripes = kernel_mode != 0 ? ((lay && atoi(lay) >= 1 && atoi(lay) <= 3) ? atoi(lay) : 3) : 0;
    ck(ctx, gv_set_layout(ctx, kernel_mode == 0, stripes), "gv_set_layout");
    ck(ctx, gv_set_kernel_mode(ctx, kernel_mode), "gv_set_kernel_mode");
    if (const char* ep = getenv("GVAMP_EXPECTED_PASSES")) ck(ctx, gv_set_expected_passes(ctx, atoll(ep) > 0 ? atoll(ep) : 0), "gv_set_expected_passes");
    if (kernel_mode == 0 && rank == 0)
        std::cerr << "WARNING: --kernel-mode 0 selects the fp64 VALU kernels (parity anchor, 4-9 % of the HBM roofline): "
                     "expect Ax / ATx 10-20x slower than the default --kernel-mode 1" << std::endl;
    if (gv_env_nranks() > 1) {
        gv_ctx* world = gv_host_world(device);          // the process's one communicator (MPI_COMM_WORLD of the reference)
        ck(ctx, gv_comm_share(ctx, world), "gv_comm_share");
    }
}

// ---- the process's communicator ------------------------------------------------------------------------------------------
// The reference has ONE MPI_COMM_WORLD per process however many `data` objects it builds (main_real --run-mode both: a training
// and a test set).  Here a small context that holds no data owns the communicator -- RCCL over xGMI by default, the shared-
// memory host transport with GVAMP_COMM=host -- and every data object's context joins it (gv_comm_share): one rendezvous per
// process, so a rendezvous file can never be read by a later object of the same run.
namespace {
gv_ctx* g_world = nullptr;
gvh_shm_comm* g_shm = nullptr;
}
gv_ctx* gv_host_world(int device) {
    if (g_world) return g_world;
    const int rank = gv_env_rank(), nranks = gv_env_nranks();
    if (device < 0) device = gv_env_local_rank();
    if (gv_create(device, &g_world)) die(std::string("FATAL: ") + gv_last_error(nullptr));
    const char* kind = getenv("GVAMP_COMM");
    if (kind && (!strcmp(kind, "host") || !strcmp(kind, "shm"))) {
        // ranks are processes of one node meeting in shared memory (shm_comm.hpp): device -> host, sum, host -> device per message
        std::string err;
        g_shm = gvh_shm_open_impl(gvh_shm_default_name(), nranks, rank, (size_t)1 << 20, err);
        if (!g_shm) die("FATAL: " + err);
        ck(g_world, gv_comm_init_callback(g_world, nranks, rank, gvh_shm_allreduce, g_shm), "gv_comm_init_callback");
        return g_world;
    }
    if (kind && strcmp(kind, "rccl") != 0) die(std::string("FATAL: GVAMP_COMM must be rccl (default) or host, not ") + kind);
    // one process per GPU: rank 0 publishes the RCCL unique id through a file whose name is private to the job -- the launcher's
    // $GVAMP_RENDEZVOUS, else derived from the launcher's job id (gvh_job_key: torchrun / Slurm / PMIx ids first, the parent's
    // pid only as the last resort)
    const std::string path = gvh_id_file_default();
    unsigned char id[128];
    if (rank == 0) ck(nullptr, gv_comm_unique_id(id), "gv_comm_unique_id");
    {
        std::string err;
        if (gvh_exchange_id_impl(path, rank, id, 60.0, err)) die("FATAL: " + err);
    }
    ck(g_world, gv_comm_init(g_world, nranks, rank, id), "gv_comm_init");   // returns after a collective: every rank has the id
    if (rank == 0) remove(path.c_str());
    return g_world;
}
// MPI_Finalize of the drivers: after the last data / vamp object is gone
void gv_host_finalize() {
    if (g_world) gv_destroy(g_world);
    g_world = nullptr;
    if (g_shm) gvh_shm_close_impl(g_shm);
    g_shm = nullptr;
}

void data::push_mask() { ck(ctx, gv_set_mask(ctx, mask4.data(), nonas), "gv_set_mask"); }

data::data(std::vector<double> y, std::string genofp, const int N, const int M, const int Mt, const int S,
           const int rank, std::string type_data, double alpha_scale, std::string bimfp, int device, int kernel_mode,
           double dosage_scale, int dosage_missing, int dosage_route)
    : bimfp(bimfp), type_data(type_data), N(N), M(M), Mt(Mt), S(S), rank(rank), phen_data(y), alpha_scale(alpha_scale),
      dosage_scale(dosage_scale), dosage_missing(dosage_missing), dosage_route(dosage_route) {
    check_type_data(type_data);
    mbytes = (N % 4) ? (size_t)N / 4 + 1 : (size_t)N / 4;
    im4 = (int)mbytes;
    mask4.assign(mbytes, 0x0F);                       // data.cpp:86-89
    if (N % 4) {                                      // data.cpp:92-98
        for (int i = N % 4; i < 4; i++) mask4[N / 4] &= ~(0b1 << i);
        std::cout << "rank = " << rank << ": setting last " << 4 - N % 4 << " bits to NAs" << std::endl;
    }
    set_nonas(N);
    open_device(device, kernel_mode);
    push_mask();
    if (type_data == "meth") {                        // data.cpp:107-110
        methfp = genofp;
        read_methylation_data();
    } else if (dosage_bits(type_data)) {
        methfp = genofp;
        read_dosage_data();
    } else {
        bedfp = genofp;
        read_genotype_data();
    }
    compute_markers_statistics();
}

data::data(std::string fp, std::string genofp, const int N, const int M, const int Mt, const int S, const int rank,
           std::string type_data, double alpha_scale, std::string bimfp, int device, int kernel_mode, double dosage_scale,
           int dosage_missing, int dosage_route)
    : phenfp(fp), bimfp(bimfp), type_data(type_data), N(N), M(M), Mt(Mt), S(S), rank(rank), alpha_scale(alpha_scale),
      dosage_scale(dosage_scale), dosage_missing(dosage_missing), dosage_route(dosage_route) {
    check_type_data(type_data);
    mbytes = (N % 4) ? (size_t)N / 4 + 1 : (size_t)N / 4;
    im4 = (int)mbytes;
    read_phen();
    open_device(device, kernel_mode);
    push_mask();
    if (type_data == "meth") {                        // data.cpp:54-57
        methfp = genofp;
        read_methylation_data();
    } else if (dosage_bits(type_data)) {
        methfp = genofp;
        read_dosage_data();
    } else {
        bedfp = genofp;
        read_genotype_data();
    }
    compute_markers_statistics();
}

data::data(gv_ctx* resident, std::vector<double> y, const int N, const int M, const int Mt, const int S, const int rank,
           const std::vector<unsigned char>* m4, int nonas_, double alpha_scale)
    : N(N), M(M), Mt(Mt), S(S), rank(rank), phen_data(y), alpha_scale(alpha_scale), ctx(resident), owns_ctx(false) {
    if (gv_get_layout(ctx) == 3) type_data = "meth";      // a dense matrix is resident
    if (gv_get_layout(ctx) == 4) type_data = "dosage8";   // ... of 8- / 16-bit dosage codes
    if (gv_get_layout(ctx) == 5) type_data = "dosage16";
    mbytes = (N % 4) ? (size_t)N / 4 + 1 : (size_t)N / 4;
    im4 = (int)mbytes;
    if (m4) {
        mask4 = *m4;
        nonas = nonas_;
    } else {
        mask4.assign(mbytes, 0x0F);
        if (N % 4)
            for (int i = N % 4; i < 4; i++) mask4[N / 4] &= ~(0b1 << i);
        nonas = N;
    }
    push_mask();
    compute_markers_statistics();
}

data::~data() {
    if (ctx && owns_ctx) gv_destroy(ctx);
}

// data.cpp:128-192: 3rd token of every line; "NA" -> DBL_MAX and mask bit cleared; scaled (not centred) by
// sqrt((nonas-1) / sum (y - mean)^2) -- NA slots are scaled too and become +inf, as in the reference.
void data::read_phen() {
    std::ifstream infile(phenfp);
    if (!infile.is_open()) die("FATAL: could not open phenotype file: " + phenfp);
    std::string line;
    double sum = 0.0;
    int line_n = 0;
    nonas = nas = 0;
    mask4.clear();
    phen_data.clear();
    while (getline(infile, line)) {
        const int k = line_n % 4;
        if (k == 0) mask4.push_back(0x0F);
        std::vector<std::string> tokens = split_ws(line);
        if (tokens.size() < 3) die("FATAL: phenotype line with fewer than 3 columns in " + phenfp);
        if (tokens[2] == "NA") {
            nas++;
            phen_data.push_back(std::numeric_limits<double>::max());
            mask4[line_n / 4] &= ~(0b1 << k);
        } else {
            nonas++;
            const double v = atof(tokens[2].c_str());
            phen_data.push_back(v);
            sum += v;
        }
        line_n++;
    }
    assert(nas + nonas == N);
    if (line_n % 4) {
        for (int i = line_n % 4; i < 4; i++) mask4[line_n / 4] &= ~(0b1 << i);
        std::cout << "rank = " << rank << ": setting last " << 4 - line_n % 4 << " bits to NAs" << std::endl;
    }
    const double avg = sum / double(nonas);
    double sqn = 0.0;
    for (double v : phen_data)
        if (v != std::numeric_limits<double>::max()) sqn += (v - avg) * (v - avg);
    sqn = sqrt(double(nonas - 1) / sqn);
    for (double& v : phen_data) v *= sqn;
    intercept = avg;
    scale = sqn;
}

// data.cpp:201-234: this rank's slab of the SNP-major .bed at byte offset 3 + S*mbytes (magic bytes skipped, not
// validated), handed to the device in bounded pieces.
void data::read_genotype_data() {
    const size_t size_bytes = size_t(M) * mbytes;
    printf("INFO   : rank %d streams %zu bytes (%.3f GB) of raw data to the device.\n", rank, size_bytes, double(size_bytes) / 1.0E9);
    const auto t0 = std::chrono::steady_clock::now();
    ck(ctx, gv_upload_bed_file(ctx, bedfp.c_str(), (int64_t)(3 + size_t(S) * mbytes)), "gv_upload_bed_file");
    if (rank == 0) {                                                                 // data.cpp:227-232
        std::cout << "reading genotype data took "
                  << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() << " seconds." << std::endl;
        gv_ingest_stats st{};
        if (gv_ingest_info2(ctx, &st) == 0 && st.layout != 0)      // [ext] what --resident-layout 3 decided, and from what
            std::cout << "resident layout: " << (st.layout == 1 ? "two stripe sets" : "one tile layout") << ", " << st.resident_bytes / 1e9
                      << " GB (expected ATx passes " << (long long)st.expected_passes
                      << (st.expected_passes >= 1000 ? ": a long run -- two sets when they fit" : ": not announced as a long run -- one layout")
                      << "; --resident-layout / GVAMP_EXPECTED_PASSES override)" << std::endl;
    }
}

// data.cpp:241-278: this rank's M x N doubles of the marker-major methylation matrix at byte offset S*N*8, handed to the
// device in bounded pieces (the reference reads them into host memory; here they go to HBM).
void data::read_methylation_data() {
    const size_t size_bytes = size_t(M) * size_t(N) * sizeof(double);
    if (rank == 0) std::cout << "meth file name = " << methfp << std::endl;
    printf("INFO   : rank %d streams %zu bytes (%.3f GB) of methylation data to the device.\n", rank, size_bytes, double(size_bytes) / 1.0E9);
    const auto t0 = std::chrono::steady_clock::now();
    ck(ctx, gv_upload_meth_file(ctx, methfp.c_str(), (int64_t)(size_t(S) * size_t(N) * sizeof(double))), "gv_upload_meth_file");
    if (rank == 0)
        std::cout << "reading methylation data took "
                  << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() << " seconds." << std::endl;
}

// [ext] compact dense data: this rank's M x N dosage codes (8 or 16 bits each, marker-major) at byte offset S*N*bits/8, streamed to
// the device as the methylation matrix is.  dosage_missing: the all-ones code is a missing entry, kept out of every sum as the bed
// path keeps a missing genotype out (gv_set_dosage_missing); otherwise every code is a value.
void data::read_dosage_data() {
    const int bits = dosage_bits(type_data);
    const size_t size_bytes = size_t(M) * size_t(N) * size_t(bits / 8);
    if (dosage_scale <= 0) dosage_scale = bits == 8 ? 1.0 / 127.0 : 1.0 / 16384.0;
    if (rank == 0)
        std::cout << "dosage file name = " << methfp << " (" << bits << "-bit codes, scale " << dosage_scale
                  << (dosage_missing ? ", the all-ones code is a missing entry)" : ")") << std::endl;
    ck(ctx, gv_set_dosage_missing(ctx, dosage_missing), "gv_set_dosage_missing");
    printf("INFO   : rank %d streams %zu bytes (%.3f GB) of dosage codes to the device.\n", rank, size_bytes, double(size_bytes) / 1.0E9);
    const auto t0 = std::chrono::steady_clock::now();
    ck(ctx, gv_upload_dosage_file(ctx, methfp.c_str(), (int64_t)(size_t(S) * size_t(N) * size_t(bits / 8)), bits, dosage_scale),
       "gv_upload_dosage_file");
    // the route of the products: a request; what is in force depends on the codes now resident (8 bits, no missing entry in this shard)
    ck(ctx, gv_set_dosage_route(ctx, dosage_route), "gv_set_dosage_route");
    int route_req = 0, route_on = 0;
    ck(ctx, gv_get_dosage_route(ctx, &route_req, &route_on), "gv_get_dosage_route");
    if (rank == 0)
        std::cout << "dosage kernels: " << (route_on ? "fixed-point i8 MFMA route" : "fp64 VALU kernels")
                  << (route_req && !route_on ? " (--dosage-kernels mfma is not in force: it needs 8-bit codes without missing entries)" : "")
                  << std::endl;
    if (rank == 0)
        std::cout << "reading dosage data took "
                  << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() << " seconds." << std::endl;
}

std::vector<int> data::read_chromosome_info(std::string bim_file) {
    std::vector<int> chroms;
    std::ifstream infile(bim_file);
    if (!infile.is_open()) die("FATAL: could not open bim file: " + bim_file);
    std::string line;
    for (int line_n = 0; getline(infile, line); line_n++) {
        if (line_n < S || line_n >= S + M) continue;
        std::vector<std::string> tokens = split_ws(line);
        if (tokens.empty()) die("FATAL: empty line " + std::to_string(line_n + 1) + " in bim file " + bim_file);
        chroms.push_back(tokens[0] == "X" ? 23 : (int)atof(tokens[0].c_str()));
    }
    return chroms;
}

void data::compute_markers_statistics() {
    const auto t0 = std::chrono::steady_clock::now();
    ck(ctx, gv_marker_stats(ctx, alpha_scale), "gv_marker_stats");
    mave.assign(M > 0 ? M : 1, 0.0);
    msig.assign(M > 0 ? M : 1, 0.0);
    ck(ctx, gv_get_marker_stats(ctx, mave.data(), msig.data()), "gv_get_marker_stats");
    if (rank == 0 && !gv_host_quiet())                                                // data.cpp:543-545
        std::cout << "rank = " << rank << ": statistics took "
                  << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() << " seconds to run."
                  << std::endl;
}

std::vector<double> data::Ax(double* __restrict__ phen) {
    std::vector<double> out(4 * mbytes, 0.0);
    ck(ctx, gv_ax(ctx, phen, out.data()), "gv_ax");
    return out;
}

std::vector<std::vector<double>> data::score(const std::vector<std::vector<double>>& cols) {
    const size_t C = cols.size(), Mp = M > 0 ? (size_t)M : 0, n4 = 4 * (size_t)mbytes;
    std::vector<double> W(C * Mp > 0 ? C * Mp : 1, 0.0), Z(C * n4 > 0 ? C * n4 : 1, 0.0);
    for (size_t j = 0; j < C; j++) {
        if (cols[j].size() != Mp) {
            std::cout << "FATAL: data::score: column " << j << " has " << cols[j].size() << " entries, the shard " << Mp << " markers" << std::endl;
            exit(EXIT_FAILURE);
        }
        std::copy(cols[j].begin(), cols[j].end(), W.begin() + j * Mp);
    }
    ck(ctx, gv_score(ctx, (int64_t)C, W.data(), Z.data()), "gv_score");
    std::vector<std::vector<double>> out(C);
    for (size_t j = 0; j < C; j++) out[j].assign(Z.begin() + j * n4, Z.begin() + (j + 1) * n4);
    return out;
}

std::vector<std::vector<double>> data::ATx_multi(const std::vector<std::vector<double>>& cols) {
    const size_t C = cols.size(), Mp = M > 0 ? (size_t)M : 0, n4 = 4 * (size_t)mbytes;
    std::vector<double> Y(C * n4 > 0 ? C * n4 : 1, 0.0), R(C * Mp > 0 ? C * Mp : 1, 0.0);
    for (size_t j = 0; j < C; j++) {
        if (cols[j].size() != n4) {
            std::cout << "FATAL: data::ATx_multi: column " << j << " has " << cols[j].size() << " entries, not 4 * mbytes = " << n4 << std::endl;
            exit(EXIT_FAILURE);
        }
        std::copy(cols[j].begin(), cols[j].end(), Y.begin() + j * n4);
    }
    ck(ctx, gv_atxm(ctx, (int64_t)C, Y.data(), R.data()), "gv_atxm");
    std::vector<std::vector<double>> out(C);
    for (size_t j = 0; j < C; j++) out[j].assign(R.begin() + j * Mp, R.begin() + (j + 1) * Mp);
    return out;
}

double data::pca_start(unsigned long long seed, unsigned long long index) {
    auto mix = [](unsigned long long z) {
        z += 0x9E3779B97F4A7C15ULL;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        return z ^ (z >> 31);
    };
    const unsigned long long base = mix(seed);
    const double u1 = ((double)(mix(base + 2 * index) >> 11) + 0.5) * 0x1p-53, u2 = ((double)(mix(base + 2 * index + 1) >> 11) + 0.5) * 0x1p-53;
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

data::pca_result data::pca(int k, int L, double tol, int max_iter, unsigned long long seed, bool loadings) {
    pca_result out;
    dev_cols q0(ctx, GV_SPACE_N, (size_t)(L > 0 ? L : 0)), u(ctx, GV_SPACE_N, (size_t)(k > 0 ? k : 0));
    std::vector<double> buf((size_t)N, 0.0);
    for (int j = 0; j < L; j++) {
        for (int n = 0; n < N; n++) buf[(size_t)n] = pca_start(seed, (unsigned long long)j * (unsigned long long)N + (unsigned long long)n);
        q0.put((size_t)j, buf);
    }
    out.eval.assign((size_t)(k > 0 ? k : 1), 0.0);
    out.resid.assign((size_t)(k > 0 ? k : 1), 0.0);
    ck(ctx, gv_pca_dev(ctx, k, L, q0.h.data(), tol, max_iter, u.h.data(), out.eval.data(), out.resid.data()), "gv_pca_dev");
    gv_pca_info(ctx, &out.info);
    for (int i = 0; i < k; i++) out.evec.push_back(u.get((size_t)i));
    if (loadings) {
        dev_cols v(ctx, GV_SPACE_M, u.h.size());
        ck(ctx, gv_pca_loadings_dev(ctx, k, u.h.data(), out.eval.data(), v.h.data()), "gv_pca_loadings_dev");
        for (int i = 0; i < k; i++) out.loadings.push_back(v.get((size_t)i));
    }
    return out;
}

data::king_result data::king_pairs(double cutoff, const std::vector<unsigned char>& use) {
    if (!use.empty() && use.size() != (size_t)(M > 0 ? M : 0)) die("FATAL: data::king_pairs: the marker selection must hold M bytes");
    king_result out;
    int64_t cap = 65536, found = 0;
    for (int round = 0; round < 2; round++) {
        out.i.assign((size_t)cap, 0);
        out.j.assign((size_t)cap, 0);
        out.kin.assign((size_t)cap, 0.0);
        out.counts.assign(5 * (size_t)cap, 0);
        ck(ctx, gv_king_pairs(ctx, use.empty() ? nullptr : use.data(), cutoff, cap, out.i.data(), out.j.data(), out.kin.data(), out.counts.data(),
                              &found), "gv_king_pairs");
        if (found <= cap) break;
        if (round == 1) die("FATAL: data::king_pairs: more pairs on the second call than the first one counted");
        cap = found;
    }
    out.i.resize((size_t)found);
    out.j.resize((size_t)found);
    out.kin.resize((size_t)found);
    out.counts.resize(5 * (size_t)found);
    gv_king_info(ctx, &out.info);
    return out;
}

data::king_result data::king_block(int64_t i0, int64_t ni, int64_t j0, int64_t nj, const std::vector<unsigned char>& use) {
    if (!use.empty() && use.size() != (size_t)(M > 0 ? M : 0)) die("FATAL: data::king_block: the marker selection must hold M bytes");
    king_result out;
    const size_t ne = ni > 0 && nj > 0 ? (size_t)ni * (size_t)nj : 0;
    out.kin.assign(ne ? ne : 1, 0.0);
    out.counts.assign(5 * (ne ? ne : 1), 0);
    ck(ctx, gv_king_block(ctx, use.empty() ? nullptr : use.data(), i0, ni, j0, nj, out.kin.data(), out.counts.data()), "gv_king_block");
    out.kin.resize(ne);
    out.counts.resize(5 * ne);
    gv_king_info(ctx, &out.info);
    return out;
}

data::grm_result data::grm_pairs(double cutoff, const std::vector<unsigned char>& use) {
    if (!use.empty() && use.size() != (size_t)(M > 0 ? M : 0)) die("FATAL: data::grm_pairs: the marker selection must hold M bytes");
    grm_result out;
    out.diag.assign((size_t)(N > 0 ? N : 1), 0.0);
    out.diag_m.assign((size_t)(N > 0 ? N : 1), 0);
    int64_t cap = 65536, found = 0;
    for (int round = 0; round < 2; round++) {
        out.i.assign((size_t)cap, 0);
        out.j.assign((size_t)cap, 0);
        out.a.assign((size_t)cap, 0.0);
        out.m_common.assign((size_t)cap, 0);
        ck(ctx, gv_grm_pairs(ctx, use.empty() ? nullptr : use.data(), cutoff, cap, out.i.data(), out.j.data(), out.a.data(), out.m_common.data(),
                             out.diag.data(), out.diag_m.data(), &found), "gv_grm_pairs");
        if (found <= cap) break;
        if (round == 1) die("FATAL: data::grm_pairs: more pairs on the second call than the first one counted");
        cap = found;
    }
    out.i.resize((size_t)found);
    out.j.resize((size_t)found);
    out.a.resize((size_t)found);
    out.m_common.resize((size_t)found);
    out.diag.resize((size_t)(N > 0 ? N : 0));
    out.diag_m.resize((size_t)(N > 0 ? N : 0));
    gv_grm_info(ctx, &out.info);
    return out;
}

data::grm_result data::grm_block(int64_t i0, int64_t ni, int64_t j0, int64_t nj, const std::vector<unsigned char>& use) {
    if (!use.empty() && use.size() != (size_t)(M > 0 ? M : 0)) die("FATAL: data::grm_block: the marker selection must hold M bytes");
    grm_result out;
    const size_t ne = ni > 0 && nj > 0 ? (size_t)ni * (size_t)nj : 0;
    out.a.assign(ne ? ne : 1, 0.0);
    out.m_common.assign(ne ? ne : 1, 0);
    ck(ctx, gv_grm_block(ctx, use.empty() ? nullptr : use.data(), i0, ni, j0, nj, out.a.data(), out.m_common.data()), "gv_grm_block");
    out.a.resize(ne);
    out.m_common.resize(ne);
    gv_grm_info(ctx, &out.info);
    return out;
}

data::grm_apply_result data::grm_apply(int C, const std::vector<double>& w, const std::vector<unsigned char>& use) {
    if (!use.empty() && use.size() != (size_t)(M > 0 ? M : 0)) die("FATAL: data::grm_apply: the marker selection must hold M bytes");
    if (C < 1 || w.size() != (size_t)N * (size_t)C) die("FATAL: data::grm_apply: the panel must hold N x C values");
    grm_apply_result out;
    out.g0.assign(w.size(), 0.0);
    out.g1.assign(w.size(), 0.0);
    out.g2.assign(w.size(), 0.0);
    ck(ctx, gv_grm_apply(ctx, use.empty() ? nullptr : use.data(), C, w.data(), out.g0.data(), out.g1.data(), out.g2.data()), "gv_grm_apply");
    gv_grm_info(ctx, &out.info);
    return out;
}

data::grm_he_result data::grm_he(int64_t C, const std::vector<double>& y, const std::vector<unsigned char>& use) {
    if (!use.empty() && use.size() != (size_t)(M > 0 ? M : 0)) die("FATAL: data::grm_he: the marker selection must hold M bytes");
    if (C < 1 || y.size() != (size_t)N * (size_t)C) die("FATAL: data::grm_he: the phenotypes must hold N x C values");
    grm_he_result out;
    out.traits.assign((size_t)C, gv_he_result{});
    ck(ctx, gv_grm_he(ctx, use.empty() ? nullptr : use.data(), C, y.data(), out.traits.data()), "gv_grm_he");
    gv_grm_info(ctx, &out.info);
    return out;
}

void data::set_mask(const std::vector<unsigned char>& m4, int nonas_) {
    if (m4.size() != mbytes) {
        std::cout << "FATAL: data::set_mask: " << m4.size() << " mask bytes, not mbytes = " << mbytes << std::endl;
        exit(EXIT_FAILURE);
    }
    mask4 = m4;
    nonas = nonas_;
    nas = N - nonas_;
    push_mask();
    compute_markers_statistics();
}

std::vector<std::vector<std::vector<double>>> data::screen(const std::vector<std::vector<double>>& cols) {
    const size_t C = cols.size(), Mp = M > 0 ? (size_t)M : 0, n4 = 4 * (size_t)mbytes;
    std::vector<std::vector<std::vector<double>>> out(3, std::vector<std::vector<double>>(C, std::vector<double>(Mp, 0.0)));
    if (C == 0) return out;
    if (nonas < 3) {
        std::cout << "FATAL: data::screen: fewer than 3 individuals with a phenotype" << std::endl;
        exit(EXIT_FAILURE);
    }
    dev_cols u(ctx, GV_SPACE_N, C), res(ctx, GV_SPACE_M, 3 * C);
    std::vector<double> buf(n4);
    for (size_t j = 0; j < C; j++) {
        if (cols[j].size() < (size_t)N) {
            std::cout << "FATAL: data::screen: column " << j << " has " << cols[j].size() << " entries, fewer than N = " << N << std::endl;
            exit(EXIT_FAILURE);
        }
        // the prepared column: zero at NA and pad slots, centred over the phenotyped, scaled by sqrt((n - 1) / sum (y - mean)^2)
        double sum = 0.0, ss = 0.0;
        for (int n = 0; n < N; n++)
            if ((mask4[n / 4] >> (n % 4)) & 1) {
                if (std::isnan(cols[j][n])) {
                    std::cout << "FATAL: data::screen: column " << j << " is NA at individual " << n << ", which the mask keeps" << std::endl;
                    exit(EXIT_FAILURE);
                }
                sum += cols[j][n];
            }
        const double avg = sum / double(nonas);
        for (int n = 0; n < N; n++)
            if ((mask4[n / 4] >> (n % 4)) & 1) ss += (cols[j][n] - avg) * (cols[j][n] - avg);
        if (!(ss > 0.0)) {
            std::cout << "FATAL: data::screen: column " << j << " has no variance over the phenotyped individuals" << std::endl;
            exit(EXIT_FAILURE);
        }
        const double sc = sqrt(double(nonas - 1) / ss);
        std::fill(buf.begin(), buf.end(), 0.0);
        for (int n = 0; n < N; n++)
            if ((mask4[n / 4] >> (n % 4)) & 1) buf[n] = (cols[j][n] - avg) * sc;
        u.put(j, buf);
    }
    gv_vec** r = res.h.data();
    ck(ctx, gv_screen_dev(ctx, (int64_t)C, u.h.data(), r, r + C, r + 2 * C), "gv_screen_dev");
    for (int k = 0; k < 3; k++)
        for (size_t j = 0; j < C && Mp > 0; j++) out[k][j] = res.get(k * C + j);
    return out;
}

void data::screen_cov_set() {
    const size_t K = covs.empty() ? 0 : covs[0].size();
    if (K > 0 && covs.size() < (size_t)N) {
        std::cout << "FATAL: data::screen_cov_set: " << covs.size() << " covariate rows, fewer than N = " << N << std::endl;
        exit(EXIT_FAILURE);
    }
    dev_cols cv(ctx, GV_SPACE_N, K);
    std::vector<double> buf((size_t)N);
    for (size_t k = 0; k < K; k++) {
        for (int n = 0; n < N; n++) buf[n] = covs[n][k];
        cv.put(k, buf);
    }
    ck(ctx, gv_screen_cov_set(ctx, (int)K, cv.h.data()), "gv_screen_cov_set");
}

std::vector<std::vector<std::vector<double>>> data::screen_cov(const std::vector<std::vector<double>>& cols, double vif_max) {
    const size_t C = cols.size(), Mp = M > 0 ? (size_t)M : 0;
    std::vector<std::vector<std::vector<double>>> out(5, std::vector<std::vector<double>>(C, std::vector<double>(Mp, 0.0)));
    if (C == 0) return out;
    dev_cols y(ctx, GV_SPACE_N, C), res(ctx, GV_SPACE_M, 5 * C);
    for (size_t j = 0; j < C; j++) {
        if (cols[j].size() < (size_t)N) {
            std::cout << "FATAL: data::screen_cov: column " << j << " has " << cols[j].size() << " entries, fewer than N = " << N << std::endl;
            exit(EXIT_FAILURE);
        }
        y.put(j, std::vector<double>(cols[j].begin(), cols[j].begin() + N));
    }
    gv_vec** r = res.h.data();
    ck(ctx, gv_screen_cov_dev(ctx, (int64_t)C, y.h.data(), vif_max, r, r + C, r + 2 * C, r + 3 * C, r + 4 * C), "gv_screen_cov_dev");
    for (int k = 0; k < 5; k++)
        for (size_t j = 0; j < C && Mp > 0; j++) out[k][j] = res.get(k * C + j);
    return out;
}

std::vector<double> data::ATx(double* __restrict__ phen) {
    std::vector<double> out(M > 0 ? M : 0, 0.0);
    ck(ctx, gv_atx(ctx, phen, out.data()), "gv_atx");
    return out;
}

// the per-chromosome predictors of data.cpp:1276-1281: <prefix>_LOCO_chr_<ch>.csv, 4*mbytes values, rank 0
static void store_chrom_pred(const std::vector<double>& pred, size_t mbytes, int rank, const std::string& pred_prefix) {
    for (int ch = 1; ch <= 23 && rank == 0; ch++) {
        const std::string fp = pred_prefix + "_LOCO_chr_" + std::to_string(ch) + ".csv";
        store_vec_to_file(fp, std::vector<double>(pred.begin() + (size_t)(ch - 1) * 4 * mbytes, pred.begin() + (size_t)ch * 4 * mbytes));
        if (!gv_host_quiet()) std::cout << "filepath predictors = " << fp << std::endl;
    }
}

std::vector<double> data::pvals_calc_dev(gv_vec* z1, gv_vec* y, gv_vec* x1_hat, bool loco, const std::string& pred_prefix) {
    std::vector<double> pv(M > 0 ? M : 1, 0.0);
    if (loco) {
        std::vector<int> ch_info = read_chromosome_info(bimfp);
        ch_info.resize(M > 0 ? M : 1, 0);
        if (pred_prefix.empty())
            ck(ctx, gv_pvals_loco(ctx, z1, y, x1_hat, ch_info.data(), pv.data()), "gv_pvals_loco");
        else {
            std::vector<double> pred((size_t)23 * 4 * mbytes, 0.0);
            ck(ctx, gv_pvals_loco_pred(ctx, z1, y, x1_hat, ch_info.data(), pv.data(), pred.data()), "gv_pvals_loco_pred");
            store_chrom_pred(pred, mbytes, rank, pred_prefix);
        }
    } else
        ck(ctx, gv_pvals_loo(ctx, z1, y, x1_hat, pv.data()), "gv_pvals_loo");
    pv.resize(M > 0 ? M : 0);
    return pv;
}

std::vector<std::vector<double>> data::assoc_calc_dev(gv_vec* z1, gv_vec* y, gv_vec* x1_hat, bool loco, const std::string& pred_prefix) {
    std::vector<std::vector<double>> res(4, std::vector<double>(M > 0 ? M : 1, 0.0));
    const gv_assoc_out out{res[0].data(), res[1].data(), res[2].data(), res[3].data()};
    if (loco) {
        std::vector<int> ch_info = read_chromosome_info(bimfp);
        ch_info.resize(M > 0 ? M : 1, 0);
        std::vector<double> pred(pred_prefix.empty() ? 0 : (size_t)23 * 4 * mbytes, 0.0);
        ck(ctx, gv_assoc_loco(ctx, z1, y, x1_hat, ch_info.data(), &out, pred.empty() ? nullptr : pred.data()), "gv_assoc_loco");
        if (!pred.empty()) store_chrom_pred(pred, mbytes, rank, pred_prefix);
    } else
        ck(ctx, gv_assoc_loo(ctx, z1, y, x1_hat, &out), "gv_assoc_loo");
    for (auto& v : res) v.resize(M > 0 ? M : 0);
    return res;
}

std::vector<std::vector<double>> data::ld_scores_dev(int window, bool adjusted) {
    std::vector<std::vector<double>> res(2, std::vector<double>(M > 0 ? M : 1, 0.0));
    std::vector<int> ch_info;
    if (bimfp != "") {
        ch_info = read_chromosome_info(bimfp);
        ch_info.resize(M > 0 ? M : 1, 0);
    }
    ck(ctx, gv_ld_scores(ctx, window, ch_info.empty() ? nullptr : ch_info.data(), adjusted ? 1 : 0, res[0].data(), res[1].data()), "gv_ld_scores");
    for (auto& v : res) v.resize(M > 0 ? M : 0);
    return res;
}

namespace {
// a whole token as a finite-or-not double; false if it is none
bool parse_double(const std::string& tok, double* out) {
    if (tok.empty()) return false;
    char* end = nullptr;
    *out = strtod(tok.c_str(), &end);
    return *end == 0;
}
}  // namespace

std::vector<double> data::read_positions(std::string bim_file, const std::string& unit) {
    const size_t col = unit == "cm" ? 2 : 3;
    std::vector<double> pos;
    std::ifstream infile(bim_file);
    if (!infile.is_open()) die("FATAL: could not open bim file: " + bim_file);
    std::string line;
    for (int line_n = 0; getline(infile, line); line_n++) {
        if (line_n < S || line_n >= S + M) continue;
        const std::vector<std::string> tokens = split_ws(line);
        double v = 0.0;
        if (tokens.size() <= col)
            die("FATAL: line " + std::to_string(line_n + 1) + " of bim file " + bim_file + " has no column " + std::to_string(col + 1) +
                " (the " + (col == 2 ? "cM" : "base-pair") + " position)");
        if (!parse_double(tokens[col], &v))
            die("FATAL: line " + std::to_string(line_n + 1) + " of bim file " + bim_file + ": \"" + tokens[col] + "\" in column " +
                std::to_string(col + 1) + " is not a number");
        pos.push_back(v);
    }
    if ((int)pos.size() != M)
        die("FATAL: bim file " + bim_file + " holds " + std::to_string(S + (int)pos.size()) + " lines, fewer than the " + std::to_string(S + M) +
            " markers");
    return pos;
}

std::vector<double> data::read_annot(std::string path, int M_, std::vector<std::string>* names) {
    std::ifstream infile(path);
    if (!infile.is_open()) die("FATAL: could not open annotation file: " + path);
    std::string line;
    if (!getline(infile, line)) die("FATAL: annotation file " + path + " is empty (line 1 must be the header)");
    std::vector<std::string> head = split_ws(line);
    if (!head.empty() && head[0].empty()) head.erase(head.begin());
    std::vector<size_t> cols;
    std::vector<std::string> cats;
    for (size_t i = 0; i < head.size(); i++)
        if (head[i] != "CHR" && head[i] != "BP" && head[i] != "SNP" && head[i] != "CM") {
            cols.push_back(i);
            cats.push_back(head[i]);
        }
    if (cols.empty()) die("FATAL: line 1 of annotation file " + path + " names no category (every column is CHR, BP, SNP or CM)");
    std::vector<double> out;
    out.reserve((size_t)M_ * cols.size());
    int rows = 0, last_line = 1;
    for (int line_n = 2; getline(infile, line); line_n++) {
        last_line = line_n;
        std::vector<std::string> tokens = split_ws(line);
        if (!tokens.empty() && tokens[0].empty()) tokens.erase(tokens.begin());
        if (tokens.empty()) continue;          // (a blank line, as at the end of the file)
        if (rows == M_)
            die("FATAL: line " + std::to_string(line_n) + " of annotation file " + path + " is row " + std::to_string(rows + 1) + ", but there are " +
                std::to_string(M_) + " markers");
        if (tokens.size() != head.size())
            die("FATAL: line " + std::to_string(line_n) + " of annotation file " + path + " has " + std::to_string(tokens.size()) + " fields, the header " +
                std::to_string(head.size()));
        for (size_t i : cols) {
            double v = 0.0;
            if (!parse_double(tokens[i], &v))
                die("FATAL: line " + std::to_string(line_n) + " of annotation file " + path + ": \"" + tokens[i] + "\" is not a number");
            if (!std::isfinite(v))
                die("FATAL: line " + std::to_string(line_n) + " of annotation file " + path + ": \"" + tokens[i] + "\" is not finite");
            out.push_back(v);
        }
        rows++;
    }
    if (rows != M_)
        die("FATAL: annotation file " + path + " ends after line " + std::to_string(last_line) + ": " + std::to_string(rows) + " rows for " +
            std::to_string(M_) + " markers");
    if (names) *names = cats;
    return out;
}

std::vector<std::vector<double>> data::ld_scores_pos_dev(const std::vector<double>& pos, double radius, bool adjusted,
                                                         const std::vector<double>& annot, int ncat) {
    const size_t C = annot.empty() ? 1 : (size_t)ncat, Mp = M > 0 ? M : 1;
    std::vector<std::vector<double>> res{std::vector<double>(Mp * C, 0.0), std::vector<double>(Mp, 0.0)};
    std::vector<int> ch_info;
    if (bimfp != "") {
        ch_info = read_chromosome_info(bimfp);
        ch_info.resize(Mp, 0);
    }
    ck(ctx, gv_ld_scores_pos(ctx, pos.data(), radius, ch_info.empty() ? nullptr : ch_info.data(), adjusted ? 1 : 0,
                             annot.empty() ? nullptr : annot.data(), ncat, res[0].data(), res[1].data()), "gv_ld_scores_pos");
    res[0].resize((size_t)(M > 0 ? M : 0) * C);
    res[1].resize(M > 0 ? M : 0);
    return res;
}

std::vector<int64_t> data::ld_clump_dev(const std::vector<double>& pos, double radius, const std::vector<double>& p, double p1, double p2,
                                        double r2, int64_t* n_index) {
    const size_t Mp = M > 0 ? M : 1;
    std::vector<int64_t> index_of(Mp, -1);
    std::vector<int> ch_info;
    if (bimfp != "") {
        ch_info = read_chromosome_info(bimfp);
        ch_info.resize(Mp, 0);
    }
    ck(ctx, gv_ld_clump(ctx, pos.data(), radius, ch_info.empty() ? nullptr : ch_info.data(), p.data(), p1, p2, r2, index_of.data(), n_index),
       "gv_ld_clump");
    index_of.resize(M > 0 ? M : 0);
    return index_of;
}

static std::vector<std::vector<double>> pvals_host(data* d, gv_ctx* ctx, std::vector<std::vector<double>>& z1, std::vector<double>& y,
                                                   std::vector<std::vector<double>>& x1_hat, bool loco,
                                                   const std::vector<std::string>& prefixes = std::vector<std::string>()) {
    std::vector<std::vector<double>> out;
    dev_cols zy(ctx, GV_SPACE_N, 2), dx(ctx, GV_SPACE_M, 1);      // z1 of the estimator at hand and y; its x1_hat
    zy.put(1, y);
    for (size_t ie = 0; ie < z1.size(); ie++) {
        zy.put(0, z1[ie]);
        dx.put(0, x1_hat[ie]);
        out.push_back(d->pvals_calc_dev(zy.h[0], zy.h[1], dx.h[0], loco, (loco && ie < prefixes.size()) ? prefixes[ie] : std::string()));
    }
    return out;
}

std::vector<std::vector<double>> data::pvals_calc(std::vector<std::vector<double>> z1, std::vector<double> y,
                                                  std::vector<std::vector<double>> x1_hat,
                                                  std::vector<std::string> filepath) {
    std::vector<std::vector<double>> pv = pvals_host(this, ctx, z1, y, x1_hat, false);
    for (size_t ie = 0; ie < pv.size() && ie < filepath.size(); ie++) mpi_store_vec_to_file(filepath[ie], pv[ie], S, M);
    return pv;
}

std::vector<std::vector<double>> data::pvals_calc_LOCO(std::vector<std::vector<double>> z1, std::vector<double> y,
                                                       std::vector<std::vector<double>> x1_hat,
                                                       std::vector<std::string> filepath) {
    std::vector<std::vector<double>> pv = pvals_host(this, ctx, z1, y, x1_hat, true, filepath);
    for (size_t ie = 0; ie < pv.size() && ie < filepath.size(); ie++)
        mpi_store_vec_to_file(filepath[ie] + "_pvals_LOCO.bin", pv[ie], S, M);          // data.cpp:1347-1350
    return pv;
}

// length 4*mbytes (the reference returns N entries and lets ATx read past the end when N % 4 != 0)
std::vector<double> data::filter_pheno() {
    std::vector<double> y(4 * mbytes, 0.0);
    for (int n = 0; n < N; n++)
        if ((mask4[n / 4] >> (n % 4)) & 1) y[n] = phen_data[n];
    return y;
}

std::vector<double> data::filter_pheno(int* nonnan) {
    std::vector<double> y = filter_pheno();
    int cnt = 0;
    for (int n = 0; n < N; n++) cnt += (mask4[n / 4] >> (n % 4)) & 1;
    *nonnan = cnt;
    return y;
}

// data.cpp:286-331 -- covariates file of the probit model: one line per individual, C whitespace-separated numbers.
// (The reference splits on the regex \s+ and dies in std::stod on a leading blank; a stream extraction reads the same
// well-formed files.)  A line with another number of values is fatal, as in the reference.
void data::read_covariates(std::string covfp, int C) {
    if (C == 0) return;
    std::ifstream covf(covfp);
    if (!covf.is_open()) {
        std::cout << "FATAL: cannot open covariates file " << covfp << std::endl;
        exit(EXIT_FAILURE);
    }
    std::string line;
    while (std::getline(covf, line)) {
        std::istringstream is(line);
        std::vector<double> entries;
        std::string tok;
        while (is >> tok) entries.push_back(std::stod(tok));
        if ((int)entries.size() != C) {
            std::cout << "FATAL: number of covariates = " << entries.size()
                      << " does not match to the specified number of covariates = " << C << std::endl;
            exit(EXIT_FAILURE);
        }
        covs.push_back(entries);
    }
    if ((int)covs.size() < N) {
        std::cout << "FATAL: covariates file " << covfp << " holds " << covs.size() << " lines for N = " << N << std::endl;
        exit(EXIT_FAILURE);
    }
}

// data.cpp:1050-1058
std::vector<double> data::Zx(std::vector<double> phen) {
    std::vector<double> out(4 * mbytes, 0.0);
    for (int i = 0; i < N; i++) out[i] = inner_prod(covs[i], phen, 0);
    return out;
}
