// trainops.h -- what trainops.hip offers the train-step runner (train_runner.hip) beyond the C ABI of pcrcg_train.h,
// declared here and nowhere else.
#pragma once
#include "common.h"

namespace pcrcg {

// element-wise pieces of the train step; rows == 0 (or n == 0) launches nothing
int tr_scale_rows(const float* src, int ld_src, const float* s, float* dst, int rows, int cols, hipStream_t st);
int tr_add_lrelu(const float* a, int lda, const float* b, int ldb, float slope, float* y, int ldy, int rows, int cols,
                 hipStream_t st);
int tr_add_lrelu_bwd(const float* y, int ldy, const float* dy, int ld_dy, float slope, float* ga, int lga, float* gb, int lgb,
                     int rows, int cols, hipStream_t st);
int tr_add2d(const float* src, int ld_src, float* dst, int ld_dst, int rows, int cols, hipStream_t st);
int tr_bias_grad(const float* dy, int ld, int rows, int cols, float* db, hipStream_t st);
int tr_l2norm_bwd(const float* x, int ldx, const float* dy, int ld_dy, float* dx, int ld_dx, int rows, int cols, hipStream_t st);
int tr_sigmoid_bwd(const float* s, const float* ds, float* dx, int ld_dx, int rows, hipStream_t st);
int tr_dot_acc(const float* a, const float* b, long n, float scale, float* out, hipStream_t st);

// InstanceNorm + LeakyReLU backward in TWO launches for tensors of few row chunks: `sums` is a ZEROED [2][c] fp64 buffer
// (the train tape keeps it in its gradient region, which one memset clears) that the statistics kernel's workgroups add to
bool instnorm_backward_sums_ok(const float* x, int n, int c, int ldx, const float* dy, int ld_dy, const float* dx, int ld_dx);
int instnorm_backward_sums(const float* x, int n, int c, int ldx, const float* stats, const float* dy, int ld_dy, float slope,
                           float* dx, int ld_dx, double* sums, hipStream_t st);

}  // namespace pcrcg
