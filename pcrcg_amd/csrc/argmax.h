// argmax.h -- the inner-product arg-max of pcrcg_feature_argmax (ref:lib/loss.py:209-213) as device bodies.  The
// single-pair kernels (trainops.hip) and the several-pairs kernels of pcrcg_inlier_stats_batch (register.hip) run the
// same code on a per-pair view, so a pair's row in a batch is bit for bit the row pcrcg_feature_argmax gives for that
// pair alone.  There is no arithmetic here that floating-point contraction could fuse (explicit fmaf, MFMA, compares),
// so the bodies mean the same under either file's -ffp-contract.
//
// Every body merges its partial winner into packed[row] with a 64-bit atomicMax on (orderable score bits, ~column): the
// larger score wins, equal scores keep the smaller column, so the result does not depend on how the columns are split.
#pragma once
#include "common.h"

namespace pcrcg {
namespace {

__device__ inline unsigned long long pack_best(float v, int j) {
    const unsigned int b = __float_as_uint(v);
    const unsigned int key = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((unsigned long long)key << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned int)j);
}

// the column of a packed winner
__device__ inline int packed_col(unsigned long long p) {
    return (int)(0xFFFFFFFFu - (unsigned int)(p & 0xFFFFFFFFull));
}

constexpr int kArgmaxTB = 128;   // B rows per LDS tile of the VALU body

// One thread owns a row of A (C floats in registers); rows of B stream through LDS (bs: kArgmaxTB * C floats) in tiles of
// kArgmaxTB rows and are read back as wave-uniform (broadcast) float4s, so the inner loop is pure FMA.  bx / by are the
// row block (256 rows) and the column range.
template <int C>
__device__ __forceinline__ void feature_argmax_valu_tile(const float* a, int lda, int n, const float* b, int ldb, int m,
                                                         int cols_per, unsigned long long* packed, float* bs, unsigned bx,
                                                         unsigned by) {
    const int row = bx * 256 + threadIdx.x;
    const int r = row < n ? row : n - 1;
    float av[C];
#pragma unroll
    for (int k = 0; k < C; ++k) av[k] = a[(long)r * lda + k];
    float bv = -INFINITY;
    int bj = 0;
    const int jbeg = by * cols_per, jend = min(m, jbeg + cols_per);
    for (int j0 = jbeg; j0 < jend; j0 += kArgmaxTB) {
        const int tj = min(kArgmaxTB, jend - j0);
        __syncthreads();
        for (int e = threadIdx.x; e < tj * C; e += 256) bs[e] = b[(long)(j0 + e / C) * ldb + e % C];
        __syncthreads();
        for (int j = 0; j < tj; ++j) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < C; k += 4) {
                const float4 v = *reinterpret_cast<const float4*>(&bs[j * C + k]);
                s = fmaf(av[k], v.x, s);
                s = fmaf(av[k + 1], v.y, s);
                s = fmaf(av[k + 2], v.z, s);
                s = fmaf(av[k + 3], v.w, s);
            }
            if (s > bv) { bv = s; bj = j0 + j; }
        }
    }
    if (row < n && jbeg < jend) atomicMax(&packed[row], pack_best(bv, bj));
}

// 32-wide descriptors on the fp32 matrix cores: a wavefront keeps 32 rows of A as its MFMA operand (lane (row, half)
// holds A[row][16 half + s]) and walks the columns of its range 32 at a time -- lane (column, half) loads the same 16
// entries of its B row as four float4 --, 16 v_mfma_f32_32x32x2_f32 per 32 x 32 block of scores; every lane keeps the
// best score and column of its 16 rows over the columns it sees (= those congruent to its lane index), strictly-greater,
// so the smaller column survives a tie; the 32 lanes of a row meet by shuffles at the end, and the column ranges through
// the atomicMax.  fp32 operands, fp32 accumulation: the reference's torch.matmul arithmetic up to summation order.
// bx / by are the row block (128 rows, 32 per wavefront) and the column range.
typedef float fa_f16 __attribute__((ext_vector_type(16)));
__device__ __forceinline__ void feature_argmax_mfma32_tile(const float* a, int lda, int n, const float* b, int ldb, int m,
                                                           int cols_per, unsigned long long* packed, unsigned bx,
                                                           unsigned by) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const int row0 = (bx * 4 + wave) * 32;
    if (row0 >= n) return;
    float av[16];
    {
        const float* ap = a + (long)min(row0 + l31, n - 1) * lda + 16 * half;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 t = *reinterpret_cast<const float4*>(ap + 4 * q);
            av[4 * q] = t.x; av[4 * q + 1] = t.y; av[4 * q + 2] = t.z; av[4 * q + 3] = t.w;
        }
    }
    float best[16];
    int bj[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { best[r] = -INFINITY; bj[r] = 0; }
    const int jbeg = by * cols_per, jend = min(m, jbeg + cols_per);
    auto load_b = [&](int j0, float4 (&t)[4]) {
        const float* bp = b + (long)min(j0 + l31, m - 1) * ldb + 16 * half;
#pragma unroll
        for (int q = 0; q < 4; ++q) t[q] = *reinterpret_cast<const float4*>(bp + 4 * q);
    };
    float4 nxt[4];
    if (jbeg < jend) load_b(jbeg, nxt);
    for (int j0 = jbeg; j0 < jend; j0 += 32) {
        const int col = j0 + l31;
        float bv[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) { bv[4 * q] = nxt[q].x; bv[4 * q + 1] = nxt[q].y; bv[4 * q + 2] = nxt[q].z; bv[4 * q + 3] = nxt[q].w; }
        if (j0 + 32 < jend) load_b(j0 + 32, nxt);           // the next block's rows are in flight behind this block's MFMAs
        fa_f16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int s2 = 0; s2 < 16; ++s2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s2], bv[s2], acc, 0, 0, 0);
        if (col < jend) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (acc[r] > best[r]) { best[r] = acc[r]; bj[r] = col; }
        }
    }
    if (jbeg >= jend) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        unsigned long long p = pack_best(best[r], bj[r]);         // (-inf, 0) from a lane that saw no column loses to any score
#pragma unroll
        for (int sh = 16; sh >= 1; sh >>= 1) {
            const unsigned long long o = __shfl_xor(p, sh, 64);
            p = o > p ? o : p;
        }
        const int row = row0 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (l31 == 0 && row < n) atomicMax(&packed[row], p);
    }
}

// any width: A rows are re-read from memory (L1/L2 resident), one thread per row
__device__ __forceinline__ void feature_argmax_any_row(const float* a, int lda, int n, const float* b, int ldb, int m, int c,
                                                       int cols_per, unsigned long long* packed, int row, unsigned by) {
    if (row >= n) return;
    float bv = -INFINITY;
    int bj = 0;
    const int jbeg = by * cols_per, jend = min(m, jbeg + cols_per);
    for (int j = jbeg; j < jend; ++j) {
        float s = 0.f;
        for (int k = 0; k < c; ++k) s = fmaf(a[(long)row * lda + k], b[(long)j * ldb + k], s);
        if (s > bv) { bv = s; bj = j; }
    }
    if (jbeg < jend) atomicMax(&packed[row], pack_best(bv, bj));
}

// the winner of a row as (column, optionally its score)
__device__ __forceinline__ void feature_argmax_unpack_row(const unsigned long long* packed, int row, long long* arg,
                                                          float* best) {
    const unsigned long long p = packed[row];
    arg[row] = (long long)(0xFFFFFFFFu - (unsigned int)(p & 0xFFFFFFFFull));
    if (best) {
        const unsigned int key = (unsigned int)(p >> 32);
        best[row] = __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
    }
}

}  // namespace
}  // namespace pcrcg
