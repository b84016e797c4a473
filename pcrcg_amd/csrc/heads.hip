// heads.hip -- the tail of PCR-CG's pose head (ref:models/architectures.py:589-596) and its gradient.
//
//   u_r = w_q h_r + b_q,  v_r = w_t h_r + b_t          h [n, 1024] = the last folding activation
//   quaternion_pred = mean_r(u_r / |u_r|),  trans_pred = mean_r(v_r)
//
// Memory-bound: h is read once (forward) and once more (backward), 4 KB per row.  No floating-point atomics: row sums
// leave every workgroup as float64 partials and a finishing launch adds them in ascending workgroup order, so two calls
// give the same bits.
//
// Forward: the seven weight rows (28 KB) sit in LDS; one wavefront serves two rows at a time (eight 16-byte loads per lane
// in flight), a lane holds columns 4 (lane + 64 j) .. + 3, the seven dot products of a row meet in a butterfly of
// __shfl_xor (a + b is commutative, so every lane ends with the same bits).  A workgroup of four wavefronts owns
// kRowsPerWg = 64 consecutive rows, sixteen per wavefront, and adds them in row order.
// Backward: no dot product is left when the forward kept u_r (q_rows), so the workgroup splits the COLUMNS: thread t owns
// columns 4t .. 4t + 3 of every row of its slab with its 28 weights in registers, and accumulates its share of dw_q and of
// sum_r h_r in float64 registers.  A slab is 64 k rows with the k that keeps the partials (41 KB per workgroup) at 512
// workgroups or fewer.
#include "common.h"
#include "pcrcg_train.h"

namespace pcrcg {
namespace {

constexpr int kWidth = 1024;           // the one width served: 64 lanes x 4 float4 (forward), 256 threads x 1 float4 (backward)
constexpr int kRowsPerWg = 64;         // forward: rows per workgroup; backward: the unit of a slab
constexpr int kThreads = 256;
constexpr int kFwdPart = 8;            // doubles per forward partial: 4 (sum of u / |u|) + 3 (sum of v) + 1 pad
constexpr int kBwdAcc = 20;            // doubles per thread of a backward partial: dw_q [4][4 columns] + sum h [4 columns]
constexpr int kBwdMaxWg = 512;

inline int fwd_groups(int n) { return (n + kRowsPerWg - 1) / kRowsPerWg; }
inline int bwd_slab(int n) {
    const int chunks = fwd_groups(n);
    return kRowsPerWg * ((chunks + kBwdMaxWg - 1) / kBwdMaxWg);
}
inline int bwd_groups(int n) {
    const int slab = bwd_slab(n);
    return (n + slab - 1) / slab;
}
inline size_t bwd_part_doubles(int groups) { return (size_t)groups * (kBwdAcc * kThreads + 4); }

__device__ __forceinline__ float dot4(const float4& a, const float4& b, float acc) {
    acc = fmaf(a.x, b.x, acc);
    acc = fmaf(a.y, b.y, acc);
    acc = fmaf(a.z, b.z, acc);
    return fmaf(a.w, b.w, acc);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// one row's seven sums (the same bits in every lane) -> its u kept, its unit quaternion and translation added to acc
__device__ __forceinline__ void finish_row(const float (&d)[7], const float (&bias)[7], float* q_rows, size_t r, int lane,
                                           double (&acc)[7]) {
    float u[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) u[k] = d[k] + bias[k];
    if (q_rows && lane == 0) reinterpret_cast<float4*>(q_rows)[r] = make_float4(u[0], u[1], u[2], u[3]);
    const double nrm = sqrt((double)u[0] * u[0] + (double)u[1] * u[1] + (double)u[2] * u[2] + (double)u[3] * u[3]);
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] += (double)u[k] / nrm;        // plain division: 0 / 0 = NaN, as torch
#pragma unroll
    for (int k = 4; k < 7; ++k) acc[k] += (double)(d[k] + bias[k]);
}

__global__ __launch_bounds__(kThreads) void k_pose_head_fwd(const float* __restrict__ h, int ld_h, int n,
                                                            const float* __restrict__ w_q, const float* __restrict__ b_q,
                                                            const float* __restrict__ w_t, const float* __restrict__ b_t,
                                                            float* __restrict__ q_rows, double* __restrict__ part) {
    __shared__ float4 sw[7][kWidth / 4];
    __shared__ double red[kThreads / kWave][kFwdPart];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < 7 * (kWidth / 4); i += kThreads) {
        const int k = i / (kWidth / 4), c = i % (kWidth / 4);
        const float* row = k < 4 ? w_q + (size_t)k * kWidth : w_t + (size_t)(k - 4) * kWidth;
        sw[k][c] = reinterpret_cast<const float4*>(row)[c];
    }
    float bias[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) bias[k] = k < 4 ? b_q[k] : b_t[k - 4];
    __syncthreads();

    const int r0 = blockIdx.x * kRowsPerWg + wave * (kRowsPerWg / 4);
    const int r1 = min(r0 + kRowsPerWg / 4, n);
    double acc[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int r = r0; r < r1; r += 2) {
        const bool two = r + 1 < r1;
        const float4* p0 = reinterpret_cast<const float4*>(h + (size_t)r * ld_h);
        const float4* p1 = reinterpret_cast<const float4*>(h + (size_t)(two ? r + 1 : r) * ld_h);
        float4 a0[4], a1[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            a0[j] = p0[lane + 64 * j];
            a1[j] = p1[lane + 64 * j];
        }
        float d0[7] = {0, 0, 0, 0, 0, 0, 0}, d1[7] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                const float4 w = sw[k][lane + 64 * j];
                d0[k] = dot4(a0[j], w, d0[k]);
                d1[k] = dot4(a1[j], w, d1[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            d0[k] = wave_sum(d0[k]);
            d1[k] = wave_sum(d1[k]);
        }
        finish_row(d0, bias, q_rows, (size_t)r, lane, acc);
        if (two) finish_row(d1, bias, q_rows, (size_t)r + 1, lane, acc);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 7; ++k) red[wave][k] = acc[k];
    }
    __syncthreads();
    if (tid < 7) part[(size_t)blockIdx.x * kFwdPart + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// sum of part[g * stride + offset], g = 0 .. groups - 1, by one wavefront: lane l adds its block of consecutive workgroups in
// order, lane 0 then adds the 64 block sums in lane order -- ascending workgroup order throughout, one fixed parenthesisation
__device__ __forceinline__ double ordered_sum(const double* part, int groups, size_t stride, size_t offset, int lane) {
    const int per = (groups + 63) / 64;
    const int g0 = min(lane * per, groups), g1 = min(g0 + per, groups);
    double s = 0.0;
    for (int g = g0; g < g1; ++g) s += part[(size_t)g * stride + offset];
    double total = 0.0;
    for (int l = 0; l < 64; ++l) total += __shfl(s, l, 64);
    return total;
}

__global__ __launch_bounds__(512) void k_pose_head_fwd_finish(const double* __restrict__ part, int groups, int n,
                                                              float* __restrict__ out7) {
    const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;        // wavefront k finishes output k (the eighth idles)
    const double total = ordered_sum(part, groups, kFwdPart, k < 7 ? k : 0, lane);
    if (k < 7 && lane == 0) out7[k] = (float)(total / (double)n);
}

__global__ __launch_bounds__(kThreads) void k_pose_head_bwd(const float* __restrict__ h, int ld_h, int n, int slab,
                                                            const float* __restrict__ w_q, const float* __restrict__ w_t,
                                                            const float* __restrict__ q_rows, const float* __restrict__ g7,
                                                            float* __restrict__ dh, int ld_dh, double* __restrict__ part,
                                                            double* __restrict__ part_db) {
    const int tid = threadIdx.x;
    float4 wq[4], wt[3];
#pragma unroll
    for (int j = 0; j < 4; ++j) wq[j] = reinterpret_cast<const float4*>(w_q + (size_t)j * kWidth)[tid];
#pragma unroll
    for (int j = 0; j < 3; ++j) wt[j] = reinterpret_cast<const float4*>(w_t + (size_t)j * kWidth)[tid];
    double gq[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) gq[j] = (double)g7[j];
    const double inv_n = 1.0 / (double)n;
    float4 ct = make_float4(0.f, 0.f, 0.f, 0.f);                     // w_t^T g_t / n on this thread's columns
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float s = (float)((double)g7[4 + j] * inv_n);
        ct.x = fmaf(wt[j].x, s, ct.x);
        ct.y = fmaf(wt[j].y, s, ct.y);
        ct.z = fmaf(wt[j].z, s, ct.z);
        ct.w = fmaf(wt[j].w, s, ct.w);
    }
    double aw[4][4], ah[4] = {0, 0, 0, 0}, adb[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) aw[j][e] = 0.0;

    const int r0 = blockIdx.x * slab, r1 = min(r0 + slab, n);        // (host: (long)groups * slab < 2^31)
    for (int r = r0; r < r1; r += 4) {
        float4 hv[4], uq[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ri = min(r + i, r1 - 1);                       // a repeated last row is loaded, never used
            hv[i] = reinterpret_cast<const float4*>(h + (size_t)ri * ld_h)[tid];
            uq[i] = reinterpret_cast<const float4*>(q_rows)[ri];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (r + i >= r1) break;
            const double u[4] = {(double)uq[i].x, (double)uq[i].y, (double)uq[i].z, (double)uq[i].w};
            const double inv = 1.0 / sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2] + u[3] * u[3]);
            const double along = (u[0] * gq[0] + u[1] * gq[1] + u[2] * gq[2] + u[3] * gq[3]) * inv;    // <u^, g_q>
            double s[4];
            float sf[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                s[j] = (gq[j] - u[j] * inv * along) * inv * inv_n;   // s_r = (I - u^ u^T) g_q / (|u| n)
                sf[j] = (float)s[j];
                adb[j] += s[j];
            }
            float4 o = ct;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                o.x = fmaf(wq[j].x, sf[j], o.x);
                o.y = fmaf(wq[j].y, sf[j], o.y);
                o.z = fmaf(wq[j].z, sf[j], o.z);
                o.w = fmaf(wq[j].w, sf[j], o.w);
            }
            reinterpret_cast<float4*>(dh + (size_t)(r + i) * ld_dh)[tid] = o;
            const double he[4] = {(double)hv[i].x, (double)hv[i].y, (double)hv[i].z, (double)hv[i].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                ah[e] += he[e];
#pragma unroll
                for (int j = 0; j < 4; ++j) aw[j][e] = fma(s[j], he[e], aw[j][e]);
            }
        }
    }
    double* mine = part + (size_t)blockIdx.x * (kBwdAcc * kThreads);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) mine[(j * 4 + e) * kThreads + tid] = aw[j][e];
#pragma unroll
    for (int e = 0; e < 4; ++e) mine[(16 + e) * kThreads + tid] = ah[e];
    if (tid == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) part_db[(size_t)blockIdx.x * 4 + j] = adb[j];
    }
}

// one thread per accumulator slot (kBwdAcc * kThreads of them) adds its slot over the workgroups in ascending order; the
// first seven threads of the launch also finish db_q and db_t
__global__ __launch_bounds__(kThreads) void k_pose_head_bwd_finish(const double* __restrict__ part,
                                                                   const double* __restrict__ part_db, int groups, int n,
                                                                   const float* __restrict__ g7, float* __restrict__ dw_q,
                                                                   float* __restrict__ db_q, float* __restrict__ dw_t,
                                                                   float* __restrict__ db_t) {
    const int slot = blockIdx.x * kThreads + threadIdx.x;            // = k * kThreads + tid of the partial layout
    const int k = slot / kThreads, tid = slot % kThreads;
    double s = 0.0;
#pragma unroll 8
    for (int g = 0; g < groups; ++g) s += part[(size_t)g * (kBwdAcc * kThreads) + slot];
    if (k < 16) {
        dw_q[(size_t)(k >> 2) * kWidth + 4 * tid + (k & 3)] = (float)s;
    } else {
        const int col = 4 * tid + (k - 16);
#pragma unroll
        for (int j = 0; j < 3; ++j) dw_t[(size_t)j * kWidth + col] = (float)((double)g7[4 + j] / (double)n * s);
    }
    if (slot < 4) {
        double b = 0.0;
        for (int g = 0; g < groups; ++g) b += part_db[(size_t)g * 4 + slot];
        db_q[slot] = (float)b;
    } else if (slot < 7) {
        db_t[slot - 4] = g7[slot];
    }
}

inline bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

}  // namespace
}  // namespace pcrcg

using namespace pcrcg;

extern "C" {

size_t pcrcg_pose_head_ws_bytes(int n, int width) {
    if (n < 1 || n > (1 << 30) || width != kWidth) {
        set_error("pcrcg_pose_head_ws_bytes: bad argument: 1 <= n <= 2^30 and width == %d", kWidth);
        return 0;
    }
    const size_t fwd = (size_t)fwd_groups(n) * kFwdPart * sizeof(double);
    const size_t bwd = bwd_part_doubles(bwd_groups(n)) * sizeof(double);
    return fwd > bwd ? fwd : bwd;
}

int pcrcg_pose_head(const float* h, int ld_h, int n, int width, const float* w_q, const float* b_q, const float* w_t,
                    const float* b_t, float* out7, float* q_rows, void* ws, size_t ws_bytes, void* stream) {
    PCRCG_CHECK_ARG(n >= 1 && n <= (1 << 30) && width == kWidth);
    PCRCG_CHECK_ARG(h && w_q && b_q && w_t && b_t && out7 && ws);
    PCRCG_CHECK_ARG(ld_h >= width && ld_h % 4 == 0);
    PCRCG_CHECK_ARG(aligned16(h) && aligned16(w_q) && aligned16(w_t) && aligned16(q_rows) && (uintptr_t)ws % 8 == 0);
    const int groups = fwd_groups(n);
    PCRCG_CHECK_ARG(ws_bytes >= (size_t)groups * kFwdPart * sizeof(double));
    hipStream_t st = as_stream(stream);
    double* part = static_cast<double*>(ws);
    hipLaunchKernelGGL(k_pose_head_fwd, dim3(groups), dim3(kThreads), 0, st, h, ld_h, n, w_q, b_q, w_t, b_t, q_rows, part);
    hipLaunchKernelGGL(k_pose_head_fwd_finish, dim3(1), dim3(512), 0, st, part, groups, n, out7);
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}

int pcrcg_pose_head_backward(const float* h, int ld_h, int n, int width, const float* w_q, const float* w_t,
                             const float* q_rows, const float* g7, float* dh, int ld_dh, float* dw_q, float* db_q, float* dw_t,
                             float* db_t, void* ws, size_t ws_bytes, void* stream) {
    PCRCG_CHECK_ARG(n >= 1 && n <= (1 << 30) && width == kWidth);
    PCRCG_CHECK_ARG(h && w_q && w_t && q_rows && g7 && dh && dw_q && db_q && dw_t && db_t && ws);
    PCRCG_CHECK_ARG(ld_h >= width && ld_h % 4 == 0 && ld_dh >= width && ld_dh % 4 == 0);
    PCRCG_CHECK_ARG(aligned16(h) && aligned16(w_q) && aligned16(w_t) && aligned16(q_rows) && aligned16(dh) &&
                    (uintptr_t)ws % 8 == 0);
    const int groups = bwd_groups(n);
    PCRCG_CHECK_ARG(ws_bytes >= bwd_part_doubles(groups) * sizeof(double));
    hipStream_t st = as_stream(stream);
    double* part = static_cast<double*>(ws);
    double* part_db = part + (size_t)groups * (kBwdAcc * kThreads);
    hipLaunchKernelGGL(k_pose_head_bwd, dim3(groups), dim3(kThreads), 0, st, h, ld_h, n, bwd_slab(n), w_q, w_t, q_rows, g7, dh,
                       ld_dh, part, part_db);
    hipLaunchKernelGGL(k_pose_head_bwd_finish, dim3(kBwdAcc), dim3(kThreads), 0, st, part, part_db, groups, n, g7, dw_q, db_q,
                       dw_t, db_t);
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}

}  // extern "C"
