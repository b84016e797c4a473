// gicp_terms_driver.cpp -- csrc/gicp_terms.h compiled for the host and run on records from a file, for
// tests/test_gicp_terms_cpu.py (which builds it with the address and undefined-behaviour sanitizers).
//
//   gicp_terms_driver terms IN OUT : IN holds records of 27 doubles (p [3], q [3], R [9] row-major, C_s [6], C_t [6]); OUT gets
//                                    the 27 terms of each
//   gicp_terms_driver cov   IN OUT : IN holds records of 4 doubles (n [3], 1 - epsilon); OUT gets the 6 covariance entries
#include <cstdio>
#include <cstring>
#include <vector>

#include "gicp_terms.h"

int main(int argc, char** argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s terms|cov IN OUT\n", argv[0]);
        return 2;
    }
    const bool terms = std::strcmp(argv[1], "terms") == 0;
    if (!terms && std::strcmp(argv[1], "cov") != 0) {
        std::fprintf(stderr, "%s: unknown mode %s\n", argv[0], argv[1]);
        return 2;
    }
    const size_t in_len = terms ? 27 : 4, out_len = terms ? 27 : 6;
    std::FILE* in = std::fopen(argv[2], "rb");
    if (!in) {
        std::perror(argv[2]);
        return 2;
    }
    std::vector<double> data;
    double buf[27];
    size_t got;
    while ((got = std::fread(buf, sizeof(double), in_len, in)) == in_len) data.insert(data.end(), buf, buf + in_len);
    std::fclose(in);
    if (got != 0) {
        std::fprintf(stderr, "%s: %s ends inside a record\n", argv[0], argv[2]);
        return 2;
    }
    std::FILE* out = std::fopen(argv[3], "wb");
    if (!out) {
        std::perror(argv[3]);
        return 2;
    }
    const size_t records = data.size() / in_len;
    for (size_t r = 0; r < records; ++r) {
        const double* rec = data.data() + r * in_len;
        double res[27];
        if (terms)
            pcrcg::gicp_terms(rec, rec + 3, rec + 6, rec + 15, rec + 21, res);
        else
            pcrcg::gicp_cov_of_normal(rec, rec[3], res);
        if (std::fwrite(res, sizeof(double), out_len, out) != out_len) {
            std::perror(argv[3]);
            return 2;
        }
    }
    if (std::fclose(out) != 0) {
        std::perror(argv[3]);
        return 2;
    }
    return 0;
}
