// conv2d.hip -- PCR-CG's 2-D image backbone, Res50UNet (ref:models/resunet.py:12-111,163-188, ref:models/resnet.py:52-135),
// as implicit-GEMM convolutions on the gfx950 matrix cores plus a handful of vectorised passes, enqueued by one C++ call.
//
// Layout.  Activations are NHWC fp32, n images stacked.  A convolution is the product C = A * B^T with rows = output
// pixels, columns = output channels and K = taps x input channels in the order (ky, kx, ci); B is the weight in the
// K-contiguous layout [cout][kh][kw][cin], derived once at pack time (pcrcg_res50unet_pack).  The A tile is gathered from
// the input by the loader -- stride and zero padding included -- so no im2col buffer exists, except for the 7x7 stem
// (cin = 3): its 147 taps are staged as [pixels][160] (zero-padded to a multiple of 32) and run as a 1x1 product.
//
// Arithmetic: the forward products' contract of include/pcrcg.h (pcrcg_gemm_set_mode, mode 1): the fp16 two-term split
// (split2h, three v_mfma_f32_32x32x16_f16 per 16-deep chunk) and, for a tile whose operands leave fp16's normal range at
// either end (a non-finite partial sum, or a row of A or B that is not all zeros but holds no value of at least 2^-14),
// the whole tile again in the exact three-term bf16 form (split2, six MFMAs per chunk).  The splits and the LDS operand
// row are gemm_x6.hip's (split_terms.h).
//
// Statistics.  Training-mode BatchNorm2d wants per-channel sums over the rows of one statistics segment -- one image
// (PCR-CG calls the backbone once per image) or all images (torch's batch statistics).  Row tiles never cross an image,
// and the epilogue adds its fp64 column sums into [segment][2][N].  Products with too few tiles to fill the device are
// split along K into partial planes; a reduction pass adds them in split order and takes the sums there.  Under
// deterministic=1 (include/pcrcg.h) no sum is added atomically: each row tile (or reduction block) stores its column sums
// as a partial, and a finishing pass adds the partials of a segment in a fixed order.
#include <algorithm>
#include <type_traits>
#include <vector>

#include "common.h"

namespace pcrcg {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

#include "split_terms.h"

constexpr int CBM = 128, CBK = 32, CNT = 256;   // row tile, k slab, threads (2 x 2 wavefronts)
constexpr int kStemK = 160;                      // 7 x 7 x 3 = 147 taps, zero-padded to a multiple of CBK

struct ConvArgs {
    const float* x;          // [n][H][W][cin]
    int H, W, cin;
    int OH, OW, KH, KW, stride, pad;
    const float* w;          // [N][K], K = KH * KW * cin
    int N, K;
    float* y;                // [n][OH][OW][N], or [n][N][OH][OW] when chw
    int mimg, tiles_m;       // rows (output pixels) per image, row tiles per image
    int k_per_split;
    float* part;             // split-K: partial planes [splits][n * mimg][N] (no statistics, no bias)
    long mtot;
    double* stats;           // [segments][2][N] column sums (sum, sum of squares); NULL: none
    double* stat_part;       // deterministic: the sums stored per (image, row tile, wave row) [n * tiles_m * 2][2][N]
                             // instead of added into stats (k_stats_finish adds them); NULL: atomics
    int per_image;           // segment = image (1) or one segment (0)
    const float* bias;       // [N] or NULL
    int chw;
};

template <int BN>
__global__ void __launch_bounds__(CNT) k_conv2d(ConvArgs a) {
    constexpr int WAVES_N = 2, WM = CBM / 2, WN = BN / WAVES_N, TM = WM / 32, TN = WN / 32;
    constexpr int A_ITERS = CBM * 4 / CNT, B_ITERS = BN * 4 / CNT;
    constexpr int A_PLANE = CBM * ROWB, B_PLANE = BN * ROWB;
    static_assert(B_ITERS >= 1 && TN >= 1, "tile too small");
    __shared__ __attribute__((aligned(16))) unsigned char smem[3 * (A_PLANE + B_PLANE)];
    __shared__ unsigned s_seen[CBM + BN];
    __shared__ int s_redo;
    unsigned char* const As = smem;
    unsigned char* const Bs = smem + 3 * A_PLANE;

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wm = wave / WAVES_N, wn = wave % WAVES_N, half = lane >> 5, l31 = lane & 31;
    const int img = blockIdx.y / a.tiles_m, m0 = (blockIdx.y % a.tiles_m) * CBM, n0 = blockIdx.x * BN;
    const int split = blockIdx.z;
    const int k_begin = split * a.k_per_split, k_end = min(a.K, k_begin + a.k_per_split);

    // this thread's A items: (output pixel, 8-channel group); the pixel's window origin is formed once
    int a_by[A_ITERS], a_bx[A_ITERS];
    bool a_ok[A_ITERS];
    const float* const xim = a.x + (long)img * a.H * a.W * a.cin;
#pragma unroll
    for (int it = 0; it < A_ITERS; ++it) {
        const int p = m0 + ((tid + it * CNT) >> 2);
        a_ok[it] = p < a.mimg;
        const int pp = min(p, a.mimg - 1), oy = pp / a.OW, ox = pp - oy * a.OW;
        a_by[it] = oy * a.stride - a.pad;
        a_bx[it] = ox * a.stride - a.pad;
    }
    f32x4 ra[A_ITERS][2], rb[B_ITERS][2];
    auto load = [&](int k0) {
        const int tap = k0 / a.cin, c0 = k0 - tap * a.cin, ky = tap / a.KW, kx = tap - ky * a.KW;   // a slab never crosses a tap
#pragma unroll
        for (int it = 0; it < A_ITERS; ++it) {
            const int iy = a_by[it] + ky, ix = a_bx[it] + kx;
            const bool ok = a_ok[it] && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            if (ok) {
                const f32x4* p = reinterpret_cast<const f32x4*>(xim + ((long)iy * a.W + ix) * a.cin + c0 + ((tid + it * CNT) & 3) * 8);
                ra[it][0] = p[0];
                ra[it][1] = p[1];
            } else {
                ra[it][0] = z;
                ra[it][1] = z;
            }
        }
#pragma unroll
        for (int it = 0; it < B_ITERS; ++it) {
            const int e = tid + it * CNT;
            const f32x4* p = reinterpret_cast<const f32x4*>(a.w + (long)min(n0 + (e >> 2), a.N - 1) * a.K + k0 + (e & 3) * 8);
            rb[it][0] = p[0];
            rb[it][1] = p[1];
        }
    };

    f32x16 acc[TM][TN], acc_lo[TM][TN];
    auto zero = [&]() {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) { acc[i][j][r] = 0.f; acc_lo[i][j][r] = 0.f; }
    };
    zero();
    float seen_a[A_ITERS], seen_b[B_ITERS];
#pragma unroll
    for (int it = 0; it < A_ITERS; ++it) seen_a[it] = 0.f;
#pragma unroll
    for (int it = 0; it < B_ITERS; ++it) seen_b[it] = 0.f;
    if (tid == 0) s_redo = 0;
    for (int i = tid; i < CBM + BN; i += CNT) s_seen[i] = 0u;

    // H2 = 1: the fp16 two-term loop (tracks each row's largest |x|); H2 = 0: the three-term bf16 loop
    auto run = [&](auto h2) {
        constexpr bool H2 = decltype(h2)::value;
        auto put = [&](unsigned char* base, int plane, int e, const f32x4* v) {
            const int row = e >> 2, kg = e & 3;
            unsigned char* d = base + row * ROWB + kg * 16;
            unsigned q1[4], q2[4], q3[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float x0 = v[j >> 1][(j & 1) * 2], x1 = v[j >> 1][(j & 1) * 2 + 1];
                if constexpr (H2) split2h(x0, x1, q1[j], q2[j]);
                else split2(x0, x1, q1[j], q2[j], q3[j]);
            }
            *reinterpret_cast<u32x4*>(d) = u32x4{q1[0], q1[1], q1[2], q1[3]};
            *reinterpret_cast<u32x4*>(d + plane) = u32x4{q2[0], q2[1], q2[2], q2[3]};
            if constexpr (!H2) *reinterpret_cast<u32x4*>(d + 2 * plane) = u32x4{q3[0], q3[1], q3[2], q3[3]};
        };
        auto amax = [](const f32x4* v, float s) {
#pragma unroll
            for (int j = 0; j < 8; ++j) s = fmaxf(s, fabsf(v[j >> 2][j & 3]));
            return s;
        };
        if (k_begin < k_end) load(k_begin);
        for (int k0 = k_begin; k0 < k_end; k0 += CBK) {
            __syncthreads();                                          // the previous slab is fully read
#pragma unroll
            for (int it = 0; it < A_ITERS; ++it) {
                if constexpr (H2) seen_a[it] = amax(ra[it], seen_a[it]);
                put(As, A_PLANE, tid + it * CNT, ra[it]);
            }
#pragma unroll
            for (int it = 0; it < B_ITERS; ++it) {
                if constexpr (H2) seen_b[it] = amax(rb[it], seen_b[it]);
                put(Bs, B_PLANE, tid + it * CNT, rb[it]);
            }
            __syncthreads();
            if (k0 + CBK < k_end) load(k0 + CBK);                     // the next slab is in flight during the products
#pragma unroll
            for (int c = 0; c < CBK / 16; ++c) {
                if constexpr (H2) {
                    f16x8 av[TM][2], bv[TN][2];
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int p = 0; p < 2; ++p)
                            av[i][p] = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(
                                As + p * A_PLANE + (wm * WM + i * 32 + l31) * ROWB + (c * 2 + half) * 16));
#pragma unroll
                    for (int j = 0; j < TN; ++j)
#pragma unroll
                        for (int p = 0; p < 2; ++p)
                            bv[j][p] = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(
                                Bs + p * B_PLANE + (wn * WN + j * 32 + l31) * ROWB + (c * 2 + half) * 16));
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j) {
                            acc_lo[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av[i][1], bv[j][0], acc_lo[i][j], 0, 0, 0);
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av[i][0], bv[j][0], acc[i][j], 0, 0, 0);
                            acc_lo[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av[i][0], bv[j][1], acc_lo[i][j], 0, 0, 0);
                        }
                } else {
                    bf16x8 av[TM][3], bv[TN][3];
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int p = 0; p < 3; ++p)
                            av[i][p] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(
                                As + p * A_PLANE + (wm * WM + i * 32 + l31) * ROWB + (c * 2 + half) * 16));
#pragma unroll
                    for (int j = 0; j < TN; ++j)
#pragma unroll
                        for (int p = 0; p < 3; ++p)
                            bv[j][p] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(
                                Bs + p * B_PLANE + (wn * WN + j * 32 + l31) * ROWB + (c * 2 + half) * 16));
#pragma unroll
                    for (int t = 0; t < 6; ++t) {        // smallest terms first: a3b1 a2b2 a1b3 | a2b1 a1b2 | a1b1
                        const int pa = (t == 0 ? 2 : t == 1 ? 1 : t == 2 ? 0 : t == 3 ? 1 : 0);
                        const int pb = (t == 0 ? 0 : t == 1 ? 1 : t == 2 ? 2 : t == 3 ? 0 : t == 4 ? 1 : 0);
#pragma unroll
                        for (int i = 0; i < TM; ++i)
#pragma unroll
                            for (int j = 0; j < TN; ++j)
                                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[i][pa], bv[j][pb], acc[i][j], 0, 0, 0);
                    }
                }
            }
        }
    };
    run(std::true_type{});
    // fp16's range, both ends (see the file head): a non-finite partial sum, or a row with values all below 2^-14
    bool bad = false;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) bad = bad || !(fabsf(acc[i][j][r]) <= 3.0e38f) || !(fabsf(acc_lo[i][j][r]) <= 3.0e38f);
    if (bad) s_redo = 1;
#pragma unroll
    for (int it = 0; it < A_ITERS; ++it)
        if (seen_a[it] > 0.f) atomicMax(&s_seen[(tid + it * CNT) >> 2], __float_as_uint(seen_a[it]));
#pragma unroll
    for (int it = 0; it < B_ITERS; ++it)
        if (seen_b[it] > 0.f) atomicMax(&s_seen[CBM + ((tid + it * CNT) >> 2)], __float_as_uint(seen_b[it]));
    __syncthreads();
    for (int i = tid; i < CBM + BN; i += CNT) {
        const unsigned v = s_seen[i];
        if (v != 0u && v < 0x38800000u) s_redo = 1;                  // 2^-14, the smallest normal fp16
    }
    __syncthreads();
    if (s_redo) {
        zero();
        run(std::false_type{});
    } else {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] += acc_lo[i][j][r] * (1.0f / kH2Scale);
    }

    // epilogue: C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const long rbase = (long)img * a.mimg;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int gn = n0 + wn * WN + j * 32 + l31;
        const float bv = (a.bias && gn < a.N) ? a.bias[gn] : 0.f;
        double s = 0.0, q = 0.0;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int gm = m0 + wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (gm < a.mimg && gn < a.N) {
                    const float v = acc[i][j][r] + bv;
                    if (a.part) a.part[((long)split * a.mtot + rbase + gm) * a.N + gn] = v;
                    else if (a.chw) a.y[((long)img * a.N + gn) * a.mimg + gm] = v;
                    else a.y[(rbase + gm) * a.N + gn] = v;
                    s += v;
                    q += (double)v * v;
                }
            }
        if (a.stats && !a.part) {
            s += __shfl_xor(s, 32, 64);
            q += __shfl_xor(q, 32, 64);
            if (half == 0 && gn < a.N) {
                if (a.stat_part) {
                    double* sp = a.stat_part + ((long)blockIdx.y * 2 + wm) * 2 * a.N;   // blockIdx.y = image, row tile
                    sp[gn] = s;
                    sp[a.N + gn] = q;
                } else {
                    double* st = a.stats + (long)(a.per_image ? img : 0) * 2 * a.N;
                    unsafeAtomicAdd(&st[gn], s);
                    unsafeAtomicAdd(&st[a.N + gn], q);
                }
            }
        }
    }
}

// split-K: y = the partial planes added in split order; statistics of the sums.  Block = (16 rows of one image, all columns).
// stat_part (deterministic): the block's sums stored at [image][block][2][N] instead of added into stats.
__global__ void k_splitk_reduce(const float* __restrict__ part, int splits, long mtot, int N, int mimg, float* __restrict__ y,
                                double* __restrict__ stats, int per_image, double* __restrict__ stat_part) {
    const int img = blockIdx.y, r0 = blockIdx.x * 16, r1 = min(mimg, r0 + 16);
    double* st = stats ? stats + (long)(per_image ? img : 0) * 2 * N : nullptr;
    for (int c = threadIdx.x; c < N; c += blockDim.x) {
        double s = 0.0, q = 0.0;
        for (int r = r0; r < r1; ++r) {
            const long row = (long)img * mimg + r;
            float v = 0.f;
            for (int k = 0; k < splits; ++k) v += part[((long)k * mtot + row) * N + c];
            y[row * N + c] = v;
            s += v;
            q += (double)v * v;
        }
        if (stat_part) {
            double* sp = stat_part + ((long)img * gridDim.x + blockIdx.x) * 2 * N;
            sp[c] = s;
            sp[N + c] = q;
        } else if (st) {
            unsafeAtomicAdd(&st[c], s);
            unsafeAtomicAdd(&st[N + c], q);
        }
    }
}

// deterministic: stats [segments][2][N] = the stored partials [n][per_img][2][N] of each segment (one image, or all) added
// in image, then partial order.  Grid (column blocks, segments).
__global__ void k_stats_finish(const double* __restrict__ part, int per_img, int n, int N, int per_image, double* __restrict__ stats) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x, seg = blockIdx.y;
    if (c >= N) return;
    const long p0 = (long)(per_image ? seg : 0) * per_img, p1 = (long)(per_image ? seg + 1 : n) * per_img;
    double s = 0.0, q = 0.0;
    for (long p = p0; p < p1; ++p) {
        s += part[p * 2 * N + c];
        q += part[p * 2 * N + N + c];
    }
    stats[(long)seg * 2 * N + c] = s;
    stats[(long)seg * 2 * N + N + c] = q;
}

// the deterministic mode's partial sums (exact size: no slack)
StreamScratch g_bn_partials;

// BatchNorm2d finalize, one thread per channel: (scale, shift) per segment into ss [segments][2][C].
//   training: batch mean, biased variance (eps) for the normalisation; running_mean / running_var updated with momentum and
//             the unbiased variance, once per segment in segment order; num_batches_tracked += segments
//   eval:     the running statistics, one segment
__global__ void k_bn_finalize(const double* __restrict__ stats, int ldn, int coff, int C, int segs, double count, int training,
                              const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ rmean,
                              float* __restrict__ rvar, long long* __restrict__ nbt, float eps, float momentum,
                              float* __restrict__ ss) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c == 0 && training && nbt) nbt[0] += segs;
    if (c >= C) return;
    const double g = gamma[c], b = beta[c];
    if (!training) {
        const double sc = g / sqrt((double)rvar[c] + (double)eps);
        ss[c] = (float)sc;
        ss[C + c] = (float)(b - (double)rmean[c] * sc);
        return;
    }
    float rm = rmean[c], rv = rvar[c];
    for (int s = 0; s < segs; ++s) {
        const double mean = stats[(long)s * 2 * ldn + coff + c] / count;
        double var = stats[(long)s * 2 * ldn + ldn + coff + c] / count - mean * mean;
        if (var < 0.0) var = 0.0;
        const double sc = g / sqrt(var + (double)eps);
        ss[(long)s * 2 * C + c] = (float)sc;
        ss[(long)s * 2 * C + C + c] = (float)(b - mean * sc);
        rm = (float)((1.0 - momentum) * rm + momentum * mean);
        rv = (float)((1.0 - momentum) * rv + momentum * var * count / (count - 1.0));
    }
    rmean[c] = rm;
    rvar[c] = rv;
}

// y = act(s1 x1 + h1 [+ x2 | + s2 x2 + h2]) [+ skip]   (BatchNorm apply, the bottleneck tail, the up-projection tail)
struct Apply {
    const float* x1; int ld1; const float* ss1;
    const float* x2; int ld2; const float* ss2;   // x2 NULL: no second term; ss2 NULL: x2 added as it is
    const float* skip;                            // [rows][C] or NULL, added after the activation
    float* y;                                     // [rows][C]
    long rows; int C; long seg_rows; int relu;
};
__global__ void k_bn_apply(Apply p) {
    const int c4s = p.C >> 2;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.rows * c4s) return;
    const long r = i / c4s;
    const int c = (int)(i - r * c4s) * 4;
    const long seg = r / p.seg_rows;
    const f32x4 x1 = *reinterpret_cast<const f32x4*>(p.x1 + r * p.ld1 + c);
    const f32x4 s1 = *reinterpret_cast<const f32x4*>(p.ss1 + seg * 2 * p.C + c);
    const f32x4 h1 = *reinterpret_cast<const f32x4*>(p.ss1 + seg * 2 * p.C + p.C + c);
    f32x4 v = s1 * x1 + h1;
    if (p.x2) {
        const f32x4 x2 = *reinterpret_cast<const f32x4*>(p.x2 + r * p.ld2 + c);
        if (p.ss2) {
            const f32x4 s2 = *reinterpret_cast<const f32x4*>(p.ss2 + seg * 2 * p.C + c);
            const f32x4 h2 = *reinterpret_cast<const f32x4*>(p.ss2 + seg * 2 * p.C + p.C + c);
            v += s2 * x2 + h2;
        } else {
            v += x2;
        }
    }
    if (p.relu) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = max_nan(v[j], 0.f);   // F.relu keeps NaN
    }
    if (p.skip) v += *reinterpret_cast<const f32x4*>(p.skip + r * p.C + c);
    *reinterpret_cast<f32x4*>(p.y + r * p.C + c) = v;
}

// 3x3 / stride 2 / pad 1 max-pool of relu(scale x + shift) (the affine before the max: a negative gamma reverses order),
// padding -inf.  x [n][H][W][C], y [n][OH][OW][C].
__global__ void k_bn_relu_maxpool(const float* __restrict__ x, int H, int W, int C, const float* __restrict__ ss, int per_image,
                                  float* __restrict__ y, int OH, int OW, int n) {
    const int c4s = C >> 2;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)n * OH * OW * c4s) return;
    const int c = (int)(i % c4s) * 4;
    long t = i / c4s;
    const int ox = (int)(t % OW);
    t /= OW;
    const int oy = (int)(t % OH), img = (int)(t / OH);
    const float* s = ss + (long)(per_image ? img : 0) * 2 * C;
    const f32x4 sc = *reinterpret_cast<const f32x4*>(s + c), sh = *reinterpret_cast<const f32x4*>(s + C + c);
    f32x4 m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int dy = 0; dy < 3; ++dy) {
        const int iy = oy * 2 - 1 + dy;
        if (iy < 0 || iy >= H) continue;
        for (int dx = 0; dx < 3; ++dx) {
            const int ix = ox * 2 - 1 + dx;
            if (ix < 0 || ix >= W) continue;
            const f32x4 v = sc * *reinterpret_cast<const f32x4*>(x + (((long)img * H + iy) * W + ix) * C + c) + sh;
#pragma unroll
            for (int j = 0; j < 4; ++j) m[j] = max_nan(m[j], max_nan(v[j], 0.f));
        }
    }
    *reinterpret_cast<f32x4*>(y + i * 4) = m;
}

// bilinear resize, align_corners=True (torch's upsample_bilinear2d arithmetic in fp32).  x [n][H][W][C] -> y [n][OH][OW][C]
__global__ void k_resize_bilinear(const float* __restrict__ x, int H, int W, int C, float* __restrict__ y, int OH, int OW, int n) {
    const int c4s = C >> 2;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)n * OH * OW * c4s) return;
    const int c = (int)(i % c4s) * 4;
    long t = i / c4s;
    const int ox = (int)(t % OW);
    t /= OW;
    const int oy = (int)(t % OH), img = (int)(t / OH);
    const float rh = OH > 1 ? (float)(H - 1) / (float)(OH - 1) : 0.f, rw = OW > 1 ? (float)(W - 1) / (float)(OW - 1) : 0.f;
    const float sy = rh * oy, sx = rw * ox;
    const int y0 = (int)sy, x0 = (int)sx;
    const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
    const float ly = sy - y0, lx = sx - x0, hy = 1.f - ly, hx = 1.f - lx;
    const float* b = x + (long)img * H * W * C + c;
    const f32x4 v00 = *reinterpret_cast<const f32x4*>(b + ((long)y0 * W + x0) * C);
    const f32x4 v01 = *reinterpret_cast<const f32x4*>(b + ((long)y0 * W + x1) * C);
    const f32x4 v10 = *reinterpret_cast<const f32x4*>(b + ((long)y1 * W + x0) * C);
    const f32x4 v11 = *reinterpret_cast<const f32x4*>(b + ((long)y1 * W + x1) * C);
    *reinterpret_cast<f32x4*>(y + i * 4) = hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
}

// the stem's staged taps: images [n][3][h][w] (CHW, the caller's layout) -> col [n * OH * OW][160], k = (ky 7 + kx) 3 + ci
__global__ void k_stem_im2col(const float* __restrict__ im, int h, int w, float* __restrict__ col, int OH, int OW, int n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)n * OH * OW * kStemK) return;
    const int k = (int)(i % kStemK);
    const long row = i / kStemK;
    const int ox = (int)(row % OW), oy = (int)(row / OW % OH), img = (int)(row / ((long)OW * OH));
    float v = 0.f;
    if (k < 147) {
        const int ci = k % 3, tap = k / 3, ky = tap / 7, kx = tap % 7;
        const int iy = oy * 2 - 3 + ky, ix = ox * 2 - 3 + kx;
        if (iy >= 0 && iy < h && ix >= 0 && ix < w) v = im[(((long)img * 3 + ci) * h + iy) * w + ix];
    }
    col[i] = v;
}

// torch [cout][cin][kh][kw] -> [row0 + cout][kh][kw][cin] of a K-contiguous arena block; the stem (cin = 3, 7 x 7) to
// [64][160] with zero padding
__global__ void k_pack_conv(const float* __restrict__ src, int cout, int cin, int kk, float* __restrict__ dst, int kpad) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)cout * kpad) return;
    const int o = (int)(i / kpad), k = (int)(i % kpad);
    float v = 0.f;
    if (k < kk * kk * cin) {
        const int tap = k / cin, ci = k % cin;
        v = src[((long)o * cin + ci) * kk * kk + tap];
    }
    dst[i] = v;
}

// ---- the network: the reference's state_dict order, 392 tensors -----------------------------------------------------------
constexpr int kTensors = 392;
constexpr int kPlanes[4] = {64, 128, 256, 512}, kBlocks[4] = {3, 4, 6, 3}, kStride[4] = {1, 2, 2, 2};

struct BnRef { int t; int C; };                               // first of its 5 tensors: weight, bias, mean, var, count
struct ConvRef { int t; int cin, cout, k, stride, pad; long aoff; int kdim; };
struct Net {
    ConvRef stem; BnRef stem_bn;
    struct Block { ConvRef c1, c2, c3, cd; BnRef b1, b2, b3, bd; bool ds; } blk[16];
    struct Up { ConvRef c1, c12, c2; BnRef b1, b12, b2; long pair_off; } up[4];
    ConvRef c0; int bias_t; long bias_off;
    long arena_floats;
    int nbn;
};

static Net make_net(int out_ch) {
    Net n{};
    int t = 0;
    long off = 0;
    auto conv = [&](int cin, int cout, int k, int stride, int pad) {
        ConvRef c{t++, cin, cout, k, stride, pad, off, k * k * cin};
        off += (long)cout * c.kdim;
        return c;
    };
    auto bn = [&](int C) { BnRef b{t, C}; t += 5; ++n.nbn; return b; };
    n.stem = conv(3, 64, 7, 2, 3);
    off -= 64L * 147;
    n.stem.kdim = kStemK;
    off += 64L * kStemK;
    n.stem_bn = bn(64);
    int inpl = 64, bi = 0;
    for (int L = 0; L < 4; ++L)
        for (int b = 0; b < kBlocks[L]; ++b, ++bi) {
            const int p = kPlanes[L], s = b == 0 ? kStride[L] : 1;
            Net::Block& B = n.blk[bi];
            B.c1 = conv(inpl, p, 1, 1, 0);
            B.b1 = bn(p);
            B.c2 = conv(p, p, 3, s, 1);
            B.b2 = bn(p);
            B.c3 = conv(p, 4 * p, 1, 1, 0);
            B.b3 = bn(4 * p);
            B.ds = b == 0;
            if (B.ds) {
                B.cd = conv(inpl, 4 * p, 1, s, 0);
                B.bd = bn(4 * p);
            }
            inpl = 4 * p;
        }
    int f = 2048;
    for (int u = 0; u < 4; ++u, f /= 2) {
        Net::Up& U = n.up[u];
        U.pair_off = off;                       // conv1 rows then conv2 rows: one [2 cout][25 cin] block
        U.c1 = conv(f, f / 2, 5, 1, 2);
        U.b1 = bn(f / 2);
        U.c12 = conv(f / 2, f / 2, 3, 1, 1);
        U.b12 = bn(f / 2);
        U.c2 = conv(f, f / 2, 5, 1, 2);
        U.b2 = bn(f / 2);
    }
    n.c0 = conv(128, out_ch, 1, 1, 0);
    n.bias_t = t++;
    n.bias_off = off;
    off += out_ch;
    n.arena_floats = off;
    return n;
}
// conv1_2 sits between conv1 and conv2 in the state_dict, but the pair must be adjacent in the arena: the layout above is
// re-based so that every up-projection stores [conv1 | conv2] first and conv1_2 after them
static void rebase_pairs(Net& n) {
    for (auto& U : n.up) {
        const long base = U.pair_off, a = (long)U.c1.cout * U.c1.kdim;
        U.c1.aoff = base;
        U.c2.aoff = base + a;
        U.c12.aoff = base + 2 * a;
    }
}
static Net net_for(int out_ch) {
    Net n = make_net(out_ch);
    rebase_pairs(n);
    return n;
}

static int ceil_half(int v) { return (v + 1) / 2; }

// The sequencer runs twice per call: `dry` only records how large every workspace buffer must be; the live pass takes
// them from the caller's workspace in the same order and launches.
struct Seq {
    bool dry;
    hipStream_t st;
    Carver* cv;
    std::vector<size_t> need;          // bytes per buffer id (dry), offsets (live)
    std::vector<char*> ptr;
    int n;
    int training, per_image;           // per_image: statistics segments = images
    size_t det_doubles;                // the deterministic mode's stored partial sums, largest product (dry pass)
    double* det_part;                  // ... and their buffer (live pass, deterministic=1 only; NULL otherwise)
    int segs() const { return training && per_image ? n : 1; }
};
enum Buf { B_COL, B_STEM, B_POOL, B_XB1, B_XB2, B_XB3, B_XB4, B_PING, B_PONG, B_T1, B_T2, B_T3, B_DS, B_R, B_P, B_T, B_U, B_D,
           B_STATS, B_PART, B_SS, B_COUNT };

template <typename T>
static T* buf(Seq& q, int id, size_t count) {
    const size_t bytes = carve_bytes(count, sizeof(T));
    if (q.dry) {
        if (bytes > q.need[id]) q.need[id] = bytes;
        return nullptr;
    }
    return reinterpret_cast<T*>(q.ptr[id]);
}

struct Dev {
    const float* arena;
    void* const* state;                // the 392 tensors (device pointers)
    float* ss_all;                     // per-BN (scale, shift) slots
    long ss_off;
};

static int split_for(int n, int mimg, int N, int K, int bn_tile) {
    const long tiles = (long)n * ((mimg + CBM - 1) / CBM) * ((N + bn_tile - 1) / bn_tile);
    if (tiles >= 256) return 1;
    const int ksteps = K / CBK;
    long s = (512 + tiles - 1) / tiles;
    s = std::min<long>(s, std::max(1, ksteps / 8));
    s = std::min<long>(s, 8);
    const long cap = (long)n << 22;
    s = std::min<long>(s, std::max<long>(1, cap / ((long)n * mimg * N)));
    return (int)std::max<long>(1, s);
}

// one convolution (+ its statistics when training): x [n][H][W][c.cin] -> y [n][OH][OW][N]
static int conv(Seq& q, const float* w, int N, const ConvRef& c, int cin, const float* x, int H, int W, float* y, int& OH,
                int& OW, const float* bias = nullptr, int chw = 0) {
    OH = (H + 2 * c.pad - c.k) / c.stride + 1;
    OW = (W + 2 * c.pad - c.k) / c.stride + 1;
    const int mimg = OH * OW, K = c.k * c.k * cin, bnt = N <= 64 ? 64 : 128;
    const int splits = chw ? 1 : split_for(q.n, mimg, N, K, bnt);
    const int kps = ((K / CBK + splits - 1) / splits) * CBK;
    const int sp = (K + kps - 1) / kps;
    const bool stats = q.training && !chw;
    double* st = buf<double>(q, B_STATS, (size_t)q.n * 2 * 2048);
    float* part = sp > 1 ? buf<float>(q, B_PART, (size_t)sp * q.n * mimg * N) : nullptr;
    const int tiles_m = (mimg + CBM - 1) / CBM, red_blocks = (mimg + 15) / 16;
    const int per_img = sp > 1 ? red_blocks : 2 * tiles_m;         // stored partial sums per image (deterministic)
    if (q.dry) {
        if (!chw) q.det_doubles = std::max(q.det_doubles, (size_t)q.n * per_img * 2 * N);
        return PCRCG_OK;
    }
    double* det = stats ? q.det_part : nullptr;
    if (stats && !det) PCRCG_CHECK_HIP(hipMemsetAsync(st, 0, sizeof(double) * q.segs() * 2 * N, q.st));
    ConvArgs a{};
    a.x = x; a.H = H; a.W = W; a.cin = cin;
    a.OH = OH; a.OW = OW; a.KH = c.k; a.KW = c.k; a.stride = c.stride; a.pad = c.pad;
    a.w = w; a.N = N; a.K = K;
    a.y = y; a.mimg = mimg; a.tiles_m = tiles_m;
    a.k_per_split = kps;
    a.part = part; a.mtot = (long)q.n * mimg;
    a.stats = stats ? st : nullptr;
    a.stat_part = sp > 1 ? nullptr : det;
    a.per_image = q.per_image;
    a.bias = bias; a.chw = chw;
    const dim3 grid((unsigned)((N + bnt - 1) / bnt), (unsigned)(q.n * a.tiles_m), (unsigned)sp);
    if (bnt == 64) hipLaunchKernelGGL(k_conv2d<64>, grid, dim3(CNT), 0, q.st, a);
    else hipLaunchKernelGGL(k_conv2d<128>, grid, dim3(CNT), 0, q.st, a);
    PCRCG_CHECK_LAUNCH();
    if (sp > 1) {
        hipLaunchKernelGGL(k_splitk_reduce, dim3((unsigned)red_blocks, (unsigned)q.n), dim3(256), 0, q.st, part, sp,
                           a.mtot, N, mimg, y, stats ? st : nullptr, q.per_image, det);
        PCRCG_CHECK_LAUNCH();
    }
    if (det) {
        hipLaunchKernelGGL(k_stats_finish, dim3((unsigned)((N + 255) / 256), (unsigned)q.segs()), dim3(256), 0, q.st, det, per_img,
                           q.n, N, q.per_image, st);
        PCRCG_CHECK_LAUNCH();
    }
    return PCRCG_OK;
}

// finalize one BatchNorm from the statistics of the last product (columns coff .. coff + C of its N); -> its ss slot
static int finalize(Seq& q, Dev& d, const BnRef& b, int N, int coff, long count_per_seg, float*& ss) {
    ss = buf<float>(q, B_SS, 0);
    if (q.dry) {
        q.need[B_SS] += carve_bytes((size_t)q.n * 2 * b.C, 4);
        return PCRCG_OK;
    }
    ss = d.ss_all + d.ss_off;
    d.ss_off += carve_bytes((size_t)q.n * 2 * b.C, 4) / 4;
    const double* st = buf<double>(q, B_STATS, 0);
    const double count = (double)count_per_seg * (q.training && !q.per_image ? q.n : 1);
    auto T = [&](int k) { return d.state[b.t + k]; };
    hipLaunchKernelGGL(k_bn_finalize, dim3((unsigned)((b.C + 255) / 256)), dim3(256), 0, q.st, st, N, coff, b.C,
                       q.training ? q.segs() : 1, count, q.training, (const float*)T(0), (const float*)T(1), (float*)T(2),
                       (float*)T(3), (long long*)T(4), 1e-5f, 0.1f, ss);
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}

static int apply(Seq& q, Apply p, long rows_per_img) {
    if (q.dry) return PCRCG_OK;
    p.rows = (long)q.n * rows_per_img;
    p.seg_rows = q.training && q.per_image ? rows_per_img : p.rows;
    const long items = p.rows * (p.C / 4);
    hipLaunchKernelGGL(k_bn_apply, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, q.st, p);
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}
static Apply mk(const float* x1, int ld1, const float* ss1, float* y, int C, int relu) {
    Apply p{};
    p.x1 = x1; p.ld1 = ld1; p.ss1 = ss1; p.y = y; p.C = C; p.relu = relu;
    return p;
}

static int sequence(Seq& q, const Net& net, Dev& d, const float* images, int h, int w, float* out, int out_ch) {
    const int n = q.n;
    const float* A = d.arena;
    int H1 = ceil_half(h), W1 = ceil_half(w), OH, OW;
    // stem: staged taps, 1x1 product, BN, relu + max-pool
    float* col = buf<float>(q, B_COL, (size_t)n * H1 * W1 * kStemK);
    float* stem = buf<float>(q, B_STEM, (size_t)n * H1 * W1 * 64);
    if (!q.dry) {
        const long items = (long)n * H1 * W1 * kStemK;
        hipLaunchKernelGGL(k_stem_im2col, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, q.st, images, h, w, col, H1, W1, n);
        PCRCG_CHECK_LAUNCH();
    }
    ConvRef one{0, kStemK, 64, 1, 1, 0, 0, kStemK};
    PCRCG_PROPAGATE(conv(q, A + net.stem.aoff, 64, one, kStemK, col, H1, W1, stem, OH, OW));
    float* ss;
    PCRCG_PROPAGATE(finalize(q, d, net.stem_bn, 64, 0, (long)H1 * W1, ss));
    const int H2 = ceil_half(H1), W2 = ceil_half(W1);
    float* pool = buf<float>(q, B_POOL, (size_t)n * H2 * W2 * 64);
    if (!q.dry) {
        const long items = (long)n * H2 * W2 * 16;
        hipLaunchKernelGGL(k_bn_relu_maxpool, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, q.st, stem, H1, W1, 64, ss,
                           q.training && q.per_image, pool, H2, W2, n);
        PCRCG_CHECK_LAUNCH();
    }
    // encoder
    const float* x = pool;
    int H = H2, W = W2, C = 64, bi = 0;
    float* xb[4];
    int xh[4], xw[4];
    for (int L = 0; L < 4; ++L) {
        for (int b = 0; b < kBlocks[L]; ++b, ++bi) {
            const Net::Block& B = net.blk[bi];
            const int p = kPlanes[L];
            float* t1 = buf<float>(q, B_T1, (size_t)n * H * W * p);
            int h1, w1, h2, w2;
            float *s1, *s2, *s3, *sd;
            PCRCG_PROPAGATE(conv(q, A + B.c1.aoff, p, B.c1, C, x, H, W, t1, h1, w1));
            PCRCG_PROPAGATE(finalize(q, d, B.b1, p, 0, (long)h1 * w1, s1));
            PCRCG_PROPAGATE(apply(q, mk(t1, p, s1, t1, p, 1), (long)h1 * w1));
            const int Ho = (H - 1) / B.c2.stride + 1, Wo = (W - 1) / B.c2.stride + 1;
            float* t2 = buf<float>(q, B_T2, (size_t)n * Ho * Wo * p);
            PCRCG_PROPAGATE(conv(q, A + B.c2.aoff, p, B.c2, p, t1, H, W, t2, h2, w2));
            PCRCG_PROPAGATE(finalize(q, d, B.b2, p, 0, (long)h2 * w2, s2));
            PCRCG_PROPAGATE(apply(q, mk(t2, p, s2, t2, p, 1), (long)h2 * w2));
            float* t3 = buf<float>(q, B_T3, (size_t)n * Ho * Wo * 4 * p);
            PCRCG_PROPAGATE(conv(q, A + B.c3.aoff, 4 * p, B.c3, p, t2, Ho, Wo, t3, h2, w2));
            PCRCG_PROPAGATE(finalize(q, d, B.b3, 4 * p, 0, (long)Ho * Wo, s3));
            const bool last = b == kBlocks[L] - 1;
            const size_t osz = (size_t)n * Ho * Wo * 4 * p;
            float* ping = buf<float>(q, B_PING, last ? 0 : osz);
            float* pong = buf<float>(q, B_PONG, last ? 0 : osz);
            float* o = last ? buf<float>(q, B_XB1 + L, osz) : (x == ping ? pong : ping);
            Apply tail = mk(t3, 4 * p, s3, o, 4 * p, 1);
            if (B.ds) {
                float* ds = buf<float>(q, B_DS, osz);
                PCRCG_PROPAGATE(conv(q, A + B.cd.aoff, 4 * p, B.cd, C, x, H, W, ds, h2, w2));
                PCRCG_PROPAGATE(finalize(q, d, B.bd, 4 * p, 0, (long)Ho * Wo, sd));
                tail.x2 = ds; tail.ld2 = 4 * p; tail.ss2 = sd;
            } else {
                tail.x2 = x; tail.ld2 = 4 * p;
            }
            PCRCG_PROPAGATE(apply(q, tail, (long)Ho * Wo));
            x = o; H = Ho; W = Wo; C = 4 * p;
        }
        xb[L] = const_cast<float*>(x);
        xh[L] = H;
        xw[L] = W;
    }
    // decoder
    const float* din = xb[3];
    int dh = xh[3], dw = xw[3], f = 2048;
    for (int u = 0; u < 4; ++u, f /= 2) {
        const Net::Up& U = net.up[u];
        const int co = f / 2, th = u < 3 ? xh[2 - u] : 2 * xh[0], tw = u < 3 ? xw[2 - u] : 2 * xw[0];
        const long px = (long)th * tw;
        float* R = buf<float>(q, B_R, (size_t)n * px * f);
        float* P = buf<float>(q, B_P, (size_t)n * px * 2 * co);
        float* T = buf<float>(q, B_T, (size_t)n * px * co);
        float* Uo = buf<float>(q, B_U, (size_t)n * px * co);
        float* D = buf<float>(q, B_D, (size_t)n * px * co);
        if (!q.dry) {
            const long items = (long)n * px * (f / 4);
            hipLaunchKernelGGL(k_resize_bilinear, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, q.st, din, dh, dw, f, R, th,
                               tw, n);
            PCRCG_CHECK_LAUNCH();
        }
        int oh, ow;
        float *s1, *s12, *s2;
        PCRCG_PROPAGATE(conv(q, A + U.c1.aoff, 2 * co, U.c1, f, R, th, tw, P, oh, ow));      // conv1 | conv2, one product
        PCRCG_PROPAGATE(finalize(q, d, U.b1, 2 * co, 0, px, s1));
        PCRCG_PROPAGATE(finalize(q, d, U.b2, 2 * co, co, px, s2));
        PCRCG_PROPAGATE(apply(q, mk(P, 2 * co, s1, T, co, 1), px));
        PCRCG_PROPAGATE(conv(q, A + U.c12.aoff, co, U.c12, co, T, th, tw, Uo, oh, ow));
        PCRCG_PROPAGATE(finalize(q, d, U.b12, co, 0, px, s12));
        Apply tail = mk(Uo, co, s12, D, co, 1);
        tail.x2 = P + co; tail.ld2 = 2 * co; tail.ss2 = s2;
        tail.skip = u < 3 ? xb[2 - u] : nullptr;
        PCRCG_PROPAGATE(apply(q, tail, px));
        din = D; dh = th; dw = tw;
    }
    int oh, ow;
    PCRCG_PROPAGATE(conv(q, A + net.c0.aoff, out_ch, net.c0, 128, din, dh, dw, out, oh, ow, A + net.bias_off, 1));
    return PCRCG_OK;
}

static bool shape_ok(int n, int h, int w, int training, int joint) {
    if (n < 1 || n > 65535 || h < 1 || w < 1 || h > 8192 || w > 8192) return false;
    if ((long)n * ceil_half(h) * ceil_half(w) * kStemK >= (1L << 31)) return false;
    int H = ceil_half(ceil_half(h)), W = ceil_half(ceil_half(w));
    for (int L = 1; L < 4; ++L) { H = ceil_half(H); W = ceil_half(W); }
    const long smallest = (long)H * W * (joint ? n : 1);   // the fewest values any statistics segment has (layer4)
    return !training || smallest >= 2;
}

static size_t plan_bytes(Seq& q, const Net& net, int h, int w, int out_ch) {
    Dev d{};
    q.need.assign(B_COUNT, 0);
    sequence(q, net, d, nullptr, h, w, nullptr, out_ch);
    size_t tot = 0;
    for (size_t b : q.need) tot += b;
    return tot;
}

}  // namespace

}  // namespace pcrcg

using namespace pcrcg;

extern "C" {

size_t pcrcg_res50unet_arena_bytes(int out_ch) {
    if (out_ch < 1 || out_ch > 4096) return 0;
    return (size_t)net_for(out_ch).arena_floats * 4;
}

int pcrcg_res50unet_pack(void* const* h_tensors, int n_tensors, int out_ch, float* arena, void* stream) {
    PCRCG_CHECK_ARG(h_tensors && arena && n_tensors == kTensors && out_ch >= 1 && out_ch <= 4096);
    for (int i = 0; i < kTensors; ++i) PCRCG_CHECK_ARG(h_tensors[i] != nullptr);
    const Net net = net_for(out_ch);
    hipStream_t st = as_stream(stream);
    auto pack = [&](const ConvRef& c, long dst_off, int kpad) -> int {
        const long items = (long)c.cout * kpad;
        hipLaunchKernelGGL(k_pack_conv, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st,
                           (const float*)h_tensors[c.t], c.cout, c.cin, c.k, arena + dst_off, kpad);
        PCRCG_CHECK_LAUNCH();
        return PCRCG_OK;
    };
    PCRCG_PROPAGATE(pack(net.stem, net.stem.aoff, kStemK));
    for (const auto& B : net.blk) {
        PCRCG_PROPAGATE(pack(B.c1, B.c1.aoff, B.c1.kdim));
        PCRCG_PROPAGATE(pack(B.c2, B.c2.aoff, B.c2.kdim));
        PCRCG_PROPAGATE(pack(B.c3, B.c3.aoff, B.c3.kdim));
        if (B.ds) PCRCG_PROPAGATE(pack(B.cd, B.cd.aoff, B.cd.kdim));
    }
    for (const auto& U : net.up) {
        PCRCG_PROPAGATE(pack(U.c1, U.c1.aoff, U.c1.kdim));
        PCRCG_PROPAGATE(pack(U.c2, U.c2.aoff, U.c2.kdim));
        PCRCG_PROPAGATE(pack(U.c12, U.c12.aoff, U.c12.kdim));
    }
    PCRCG_PROPAGATE(pack(net.c0, net.c0.aoff, net.c0.kdim));
    PCRCG_CHECK_HIP(hipMemcpyAsync(arena + net.bias_off, h_tensors[net.bias_t], sizeof(float) * out_ch, hipMemcpyDeviceToDevice, st));
    return PCRCG_OK;
}

size_t pcrcg_res50unet_ws_bytes(int n_images, int h, int w) {
    if (!shape_ok(n_images, h, w, 0, 0)) return 0;
    Seq q{};
    q.dry = true;
    q.n = n_images;
    q.training = 1;          // the largest form: per-image statistics
    q.per_image = 1;
    return plan_bytes(q, net_for(128), h, w, 128);
}

int pcrcg_res50unet_forward(const float* arena, void* const* h_state, int n_tensors, int out_ch, const float* images,
                            int n_images, int h, int w, int joint_stats, int training, float* out, void* ws, size_t ws_bytes,
                            void* stream) {
    PCRCG_CHECK_ARG(arena && h_state && images && out && ws && n_tensors == kTensors && out_ch >= 1 && out_ch <= 4096);
    PCRCG_CHECK_ARG(joint_stats == 0 || joint_stats == 1);
    PCRCG_CHECK_ARG(training == 0 || training == 1);
    PCRCG_CHECK_ARG(shape_ok(n_images, h, w, training, joint_stats));
    for (int i = 0; i < kTensors; ++i) PCRCG_CHECK_ARG(h_state[i] != nullptr);
    const Net net = net_for(out_ch);
    Seq q{};
    q.dry = true;
    q.n = n_images;
    q.training = 1;
    q.per_image = 1;
    plan_bytes(q, net, h, w, out_ch);      // the workspace layout pcrcg_res50unet_ws_bytes reports
    Carver cv(ws, ws_bytes);
    q.ptr.assign(B_COUNT, nullptr);
    for (int b = 0; b < B_COUNT; ++b) q.ptr[b] = cv.take<char>(q.need[b]);
    PCRCG_CHECK_WS(cv);
    q.dry = false;
    q.st = as_stream(stream);
    q.training = training;
    q.per_image = !joint_stats;
    if (training && debug_opts().deterministic) {         // no floating-point atomics: the sums' partials, stored
        q.det_part = static_cast<double*>(g_bn_partials.get(q.st, q.det_doubles * sizeof(double)));
        if (!q.det_part) {
            set_error("pcrcg_res50unet_forward: deterministic=1 could not allocate %zu bytes of partial sums", q.det_doubles * 8);
            return PCRCG_ELAUNCH;
        }
    }
    Dev d{arena, h_state, reinterpret_cast<float*>(q.ptr[B_SS]), 0};
    return sequence(q, net, d, images, h, w, out, out_ch);
}
}
