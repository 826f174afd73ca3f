// driver_common.hpp -- what the two real-data drivers (main_real.cpp, main_real_probit.cpp) both do, once.
#pragma once
#include <cstdlib>
#include <iostream>

#include "utilities.hpp"

// ".bin" = raw doubles at offset S*8 (mpi_read_vec_from_file), anything else = text, one value per line
inline std::vector<double> load_estimate(const std::string& file, int M, int S) {
    const size_t dot = file.find(".");
    const std::string ext = dot == std::string::npos ? "" : file.substr(dot + 1);
    std::vector<double> x = (ext == "bin") ? mpi_read_vec_from_file(file, M, S) : read_vec_from_file(file, M, S);
    x.resize(M, 0.0);
    return x;
}

inline void need_phen(const std::vector<std::string>& files, const char* flag) {
    if (!files.empty()) return;
    std::cout << "FATAL  : no phen file(s) provided! Please use the " << flag << " option." << std::endl;
    exit(EXIT_FAILURE);
}

// this rank's share of Mt markers: M of them from marker S on (divide_work prints its INFO line here)
struct Shard {
    int M, S;
};
inline Shard shard_of(int Mt) {
    const std::vector<double> MS = divide_work(Mt);
    return {(int)MS[0], (int)MS[1]};
}

// the estimate file of iteration `it`: what precedes the "it" at pos_it of the --estimate-file, then it_<it>.<ext>
inline std::string iteration_file(const std::string& est, size_t pos_it, const std::string& ext, int it) {
    return est.substr(0, pos_it) + "it_" + std::to_string(it) + "." + ext;
}
