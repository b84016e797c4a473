// colored_terms_driver.cpp -- csrc/colored_terms.h and csrc/smallsolve.h's solve_ldlt3 compiled for the host and run on records
// from a file, for tests/test_colored_terms_cpu.py (which builds it with the address and undefined-behaviour sanitizers).
//
//   colored_terms_driver terms IN OUT : IN holds records of 17 doubles (p [3], q [3], rec [8], Is, sg, sp); OUT gets the 27 terms
//   colored_terms_driver row   IN OUT : IN holds records of 11 doubles (vt [3], nt [3], a [3], Ia, Ik); OUT gets the 9 products
//   colored_terms_driver fit   IN OUT : IN holds records of 13 doubles (sums [9], nt [3], nn); OUT gets 13 per record: the 9
//                                       sums with the last row added, the flag (1 / 0) of solve_ldlt3 and g (kUntouched where
//                                       the solve refused)
#include <cstdio>
#include <cstring>
#include <vector>

#include "colored_terms.h"
#include "smallsolve.h"

static const double kUntouched = -12345.0;

int main(int argc, char** argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s terms|row|fit IN OUT\n", argv[0]);
        return 2;
    }
    const int mode = std::strcmp(argv[1], "terms") == 0 ? 0 : std::strcmp(argv[1], "row") == 0 ? 1 : std::strcmp(argv[1], "fit") == 0 ? 2 : -1;
    if (mode < 0) {
        std::fprintf(stderr, "%s: unknown mode %s\n", argv[0], argv[1]);
        return 2;
    }
    const size_t in_len = mode == 0 ? 17 : mode == 1 ? 11 : 13, out_len = mode == 0 ? 27 : mode == 1 ? 9 : 13;
    std::FILE* in = std::fopen(argv[2], "rb");
    if (!in) {
        std::perror(argv[2]);
        return 2;
    }
    std::vector<double> data;
    double buf[17];
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
        if (mode == 0) {
            pcrcg::colored_terms(rec, rec + 3, rec + 6, rec[14], rec[15], rec[16], res);
        } else if (mode == 1) {
            pcrcg::colored_gradient_row(rec, rec + 3, rec + 6, rec[9], rec[10], res);
        } else {
            for (int e = 0; e < 9; ++e) res[e] = rec[e];
            pcrcg::colored_gradient_last_row(rec + 9, (int)rec[12], res);
            res[10] = res[11] = res[12] = kUntouched;
            res[9] = pcrcg::solve_ldlt3(res, res + 6, res + 10) ? 1.0 : 0.0;
        }
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
