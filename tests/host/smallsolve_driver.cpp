// smallsolve_driver.cpp -- csrc/smallsolve.h compiled for the host and run on records from a file, for
// tests/test_smallsolve_cpu.py (which builds it with the address and undefined-behaviour sanitizers).
//
//   smallsolve_driver ldlt6 IN OUT : IN holds records of 27 doubles (A's upper triangle row by row, then b); OUT gets 7
//                                    doubles per record: the flag (1 / 0) and x
//   smallsolve_driver eig3  IN OUT : IN holds records of 6 doubles (xx xy xz yy yz zz); OUT gets 4 per record: flag and n
//
// x and n are filled with kUntouched before every call, so a caller sees whether a refusing call left them alone.
#include <cstdio>
#include <cstring>
#include <vector>

#include "smallsolve.h"

static const double kUntouched = -12345.0;

int main(int argc, char** argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s ldlt6|eig3 IN OUT\n", argv[0]);
        return 2;
    }
    const bool ldlt = std::strcmp(argv[1], "ldlt6") == 0;
    if (!ldlt && std::strcmp(argv[1], "eig3") != 0) {
        std::fprintf(stderr, "%s: unknown solver %s\n", argv[0], argv[1]);
        return 2;
    }
    const size_t in_len = ldlt ? 27 : 6, out_len = ldlt ? 6 : 3;
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
        double res[7];
        for (size_t e = 0; e < out_len; ++e) res[1 + e] = kUntouched;
        const bool ok = ldlt ? pcrcg::solve_ldlt6(rec, rec + 21, res + 1) : pcrcg::smallest_eigenvector_sym3(rec, res + 1);
        res[0] = ok ? 1.0 : 0.0;
        if (std::fwrite(res, sizeof(double), 1 + out_len, out) != 1 + out_len) {
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
