// robust_kernel_driver.cpp -- csrc/robust_kernel.h and csrc/colored_terms.h's colored_terms_robust compiled for the host and run
// on records from a file, for tests/test_robust_kernel_cpu.py (which builds it with the address and undefined-behaviour
// sanitizers).
//
//   robust_kernel_driver weight  IN OUT : IN holds records of 3 doubles (kind, k, r); OUT gets robust_weight(kind, k, r)
//   robust_kernel_driver plane   IN OUT : IN holds records of 11 doubles (p [3], q [3], n [3], kind, k); OUT gets the 27 terms of
//                                         plane_terms_robust
//   robust_kernel_driver colored IN OUT : IN holds records of 19 doubles (p [3], q [3], rec [8], Is, sg, sp, kind, k); OUT gets
//                                         the 27 terms of colored_terms_robust
//   robust_kernel_driver plain   IN OUT : the records of `colored` (kind and k are not read); OUT gets the 27 terms of colored_terms
#include <cstdio>
#include <cstring>
#include <vector>

#include "colored_terms.h"
#include "robust_kernel.h"

int main(int argc, char** argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s weight|plane|colored|plain IN OUT\n", argv[0]);
        return 2;
    }
    static const char* const kModes[4] = {"weight", "plane", "colored", "plain"};
    int mode = -1;
    for (int m = 0; m < 4; ++m)
        if (std::strcmp(argv[1], kModes[m]) == 0) mode = m;
    if (mode < 0) {
        std::fprintf(stderr, "%s: unknown mode %s\n", argv[0], argv[1]);
        return 2;
    }
    const size_t in_len = mode == 0 ? 3 : mode == 1 ? 11 : 19, out_len = mode == 0 ? 1 : 27;
    std::FILE* in = std::fopen(argv[2], "rb");
    if (!in) {
        std::perror(argv[2]);
        return 2;
    }
    std::vector<double> data;
    double buf[19];
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
            res[0] = pcrcg::robust_weight((int)rec[0], rec[1], rec[2]);
        } else if (mode == 1) {
            pcrcg::plane_terms_robust(rec, rec + 3, rec + 6, (int)rec[9], rec[10], res);
        } else if (mode == 2) {
            pcrcg::colored_terms_robust(rec, rec + 3, rec + 6, rec[14], rec[15], rec[16], (int)rec[17], rec[18], res);
        } else {
            pcrcg::colored_terms(rec, rec + 3, rec + 6, rec[14], rec[15], rec[16], res);
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
