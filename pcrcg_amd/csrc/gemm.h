// gemm.h -- the internal GEMM interface of libpcrcg_hip.so, declared here and nowhere else: the descriptor of one product
// (GemmCall), the one entry that runs it (gemm_run, gemm.hip) and what gemm.hip and gemm_x6.hip need of each other.
// The network runners fill a GemmCall; the extern "C" entries of gemm.hip do the same with their arguments.
#pragma once
#include "common.h"

namespace pcrcg {

// optional extras of a C = A * B^T product (the decoder's fused upsample + concat, runner.hip); gemm_x6.hip only
struct GemmExtra {
    const long long* a_idx = nullptr;   // != NULL: output row r reads A row a_idx[r * a_idx_ld] (first column of a table)
    int a_idx_ld = 0, a_ns = 0;         // an index outside [0, a_ns) reads a_zero instead (the shadow row)
    const float* a_zero = nullptr;      // >= k zero floats
    bool accumulate = false;            // C += product (fp32 atomics) instead of C = product
    const double* a_sums = nullptr;     // != NULL: A is normalised on load, a' = lrelu((a - mean_k) * rstd_k, a_slope), with
    double a_count = 0.0;               // the statistics of its columns given as fp64 sums [2][k] over a_count rows
    float a_eps = 1e-5f, a_slope = 1.0f;
    int grad_operand = 0;               // train step: 1 = A holds gradients, 2 = B does (the fp16 form scales that operand by 2^16)
};

// a SECOND product C1 = f(A1) * B^T that shares B (and the bias, the leading dimensions, n, k and every GemmExtra setting
// except the per-product pointers below) with the first and runs in the SAME launch: the same layer of a second fragment
// pair (runner.hip, pcrcg_kpfcnn_forward_group).  Small products fill the chip twice as well and every product costs one
// launch per two pairs.  gemm_x6.hip only.
struct GemmPair {
    const float* a = nullptr;
    float* c = nullptr;
    int m = 0;
    const float* row_scale = nullptr;
    void* colstats = nullptr;           // statistics of C1, same form and size as the first product's
    int* h_chunks = nullptr;
    bool c_zeroed = false;
    const long long* a_idx = nullptr;   // gather form: its own table and source row count (A1 = its source matrix)
    int a_ns = 0;
    const double* a_sums = nullptr;     // normalise-on-load form: its own column sums and row count
    double a_count = 0.0;
};
struct GemmGroup {                      // up to 3 further products in the launch (4 fragment pairs per call)
    int n = 0;
    GemmPair p[3];
};

enum class GemmA { row_f32, kmajor_f32, row_bf16 };   // A stored [M, K] fp32 / [K, M] fp32 (A^T given) / [M, K] bf16
enum class GemmB { nk, kn };                          // B stored [N, K] (C = A * B^T: weights) / [K, N] (C = A * B)

// One product  C (+)= (op(A) * op(B)) * row_scale[m] + bias[n]  with everything that may ride along.
struct GemmCall {
    const void* a = nullptr;            // fp32, or bf16 with GemmA::row_bf16 (lda in bf16 elements, 16-byte aligned rows, k % 32 == 0)
    const float* b = nullptr;
    float* c = nullptr;
    int lda = 0, ldb = 0, ldc = 0;
    int m = 0, n = 0, k = 0;
    GemmA a_form = GemmA::row_f32;
    GemmB b_form = GemmB::nk;
    const float* row_scale = nullptr;   // [m] or NULL
    const float* bias = nullptr;        // [n] or NULL
    // Column statistics of C from the product's epilogue (InstanceNorm), left only when every element is written exactly once.
    // *h_chunks on return: 0 nothing was left, > 0 that many fp64 partial chunks [2][n][chunks] in `colstats`, -1 (asked for
    // with colstats_sums: `colstats` is a ZEROED [2][n] fp64 accumulator) the column sums were added there with atomics.
    void* colstats = nullptr;
    size_t colstats_bytes = 0;
    int* h_chunks = nullptr;
    bool colstats_sums = false;
    bool c_zeroed = false;              // C is all zeros already (the runner's zero arena): a split-K product skips its memset
    const GemmExtra* ex = nullptr;      // with the split-term arithmetic only, like grp
    const GemmGroup* grp = nullptr;     // NULL or n == 0: a single product
    hipStream_t st = nullptr;
};

// gemm.hip.  Checks the call, then runs it: on gemm_x6.hip's kernels when the split-term arithmetic is on (and for a bf16 A
// always), else on the fp32-MFMA kernel, which knows neither extras nor groups (PCRCG_EBADARG) nor the sums form of the
// statistics (*h_chunks = 0).  A^T * B^T is always fp32-MFMA.
int gemm_run(const GemmCall& g);
// Arithmetic mode 1 (pcrcg_gemm_set_mode, the default): fp32 operands as exact sums of bf16 / fp16 terms on the matrix cores
bool gemm_split_terms_on();
// Does a C = A * B^T product of this shape accumulate split-K partial sums into C (so that a C taken from the runner's
// pre-zeroed arena saves the product's own memset)?  m: rows of the largest product of a grouped launch, m_total: of all.
bool gemm_bt_accumulates(int m, int n, int k, long m_total = 0);

// gemm_x6.hip, for gemm.hip: a checked call on the split-term kernels; the split-K factor its plan gives an A * B^T product
int gemm_x6_dispatch(const GemmCall& g);
int gemm_x6_splits(int m, int n, int k, long m_total);
int gemm_x6_redo_counts(unsigned long long* out, int reset);
// the calling host thread enqueues beside other streams (see x6_plan_for; C ABI: pcrcg_thread_shares_gpu)
bool gemm_x6_shared();
void gemm_x6_set_shared(int on);

}  // namespace pcrcg
