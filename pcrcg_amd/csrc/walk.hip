// walk.hip -- the order in which the gather kernels visit their queries (kpconv.hip: k_kpconv_mfma, pointops.hip:
// k_gather_max).  Nothing moves in memory: a walk is a PERMUTATION OF QUERY INDICES, walk[pos] = q, sorted by a coarse
// 12-bit Morton key of the query's cell in a 16 x 16 x 16 grid over the cloud's bounding box.  The gather kernels give
// XCD x the x-th eighth of the positions (workgroup b runs on XCD b mod 8), so each of the eight private L2s serves one
// compact part of the cloud instead of queries scattered over all of it, and a support row is fetched by one or two L2s
// instead of up to eight.  Each output row is computed exactly as without a walk: results are bit-identical.
//
// One workgroup of 1024 threads per cloud (latency work, once per level and forward call): bounding box, LDS histogram
// over the 4096 keys, scan, scatter through LDS cursors.  The order INSIDE a bin depends on the atomics' arrival; only the
// processing order of the gathers depends on it, never a result.
//
// This file builds walks (k_query_walk, query_walk_multi, pcrcg_query_walk) and holds the max-pool entry that takes one;
// the KPConv gather's entries that take one are with the gather's other entries in kpconv.hip.
#include <cfloat>

#include "block_scan.h"
#include "common.h"

namespace pcrcg {
namespace {

constexpr int kWalkThreads = 1024;
constexpr int kWalkBins = 4096;

struct WalkMulti { const float* pts[4]; int* walk[4]; int* key[4]; int n[4]; };

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= FLT_MAX; }      // false for NaN and +-inf

// cell of one coordinate: 0 .. 15; NaN or infinite coordinates go to cell 0
__device__ __forceinline__ int walk_cell(float p, float lo, float scale) {
    const float v = finite_f(p) ? (p - lo) * scale : 0.f;
    return !(v >= 0.f) ? 0 : (v < 15.f ? (int)v : 15);
}
// bits 0 .. 3 of c to bits 0, 3, 6, 9
__device__ __forceinline__ int spread3(int c) { return (c & 1) | ((c & 2) << 2) | ((c & 4) << 4) | ((c & 8) << 6); }

__device__ __forceinline__ int walk_key(const float* p, const float* lo, const float* scale) {
    return spread3(walk_cell(p[0], lo[0], scale[0])) | (spread3(walk_cell(p[1], lo[1], scale[1])) << 1) |
           (spread3(walk_cell(p[2], lo[2], scale[2])) << 2);
}

// One workgroup reads the whole cloud three times, so what bounds the kernel is how many loads it keeps in flight: every
// thread fetches kWalkBatch points (clamped addresses, all loads issued before the first use) per step.
constexpr int kWalkBatch = 8;
__device__ __forceinline__ void walk_fetch(const float* __restrict__ pts, int i0, int n, float (&v)[kWalkBatch][3]) {
#pragma unroll
    for (int u = 0; u < kWalkBatch; ++u) {
        const int i = i0 + u * kWalkThreads;
        const long ic = i < n ? i : n - 1;
#pragma unroll
        for (int a = 0; a < 3; ++a) v[u][a] = pts[3 * ic + a];
    }
}

__global__ void __launch_bounds__(kWalkThreads) k_query_walk(WalkMulti mm) {
    __shared__ int s_bin[kWalkBins];
    __shared__ float s_red[kWalkThreads / 64][6];
    __shared__ float s_lo[3], s_scale[3];
    __shared__ int s_scan[kWalkThreads / 64];
    const int g = blockIdx.x;
    const float* __restrict__ pts = mm.pts[g];
    int* __restrict__ walk = mm.walk[g];
    int* __restrict__ key_out = mm.key[g];
    const int n = mm.n[g];
    if (n <= 0) return;                       // (uniform: the whole workgroup leaves)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // 1. bounding box of the finite coordinates
    float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    float v[kWalkBatch][3];
    for (int i0 = tid; i0 < n; i0 += kWalkBatch * kWalkThreads) {
        walk_fetch(pts, i0, n, v);              // (a clamped repeat of the last point changes no minimum)
#pragma unroll
        for (int u = 0; u < kWalkBatch; ++u)
#pragma unroll
            for (int a = 0; a < 3; ++a)
                if (finite_f(v[u][a])) { lo[a] = fminf(lo[a], v[u][a]); hi[a] = fmaxf(hi[a], v[u][a]); }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], d, 64));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], d, 64));
        }
    if (lane == 0)
#pragma unroll
        for (int a = 0; a < 3; ++a) { s_red[wave][a] = lo[a]; s_red[wave][3 + a] = hi[a]; }
    for (int b = tid; b < kWalkBins; b += kWalkThreads) s_bin[b] = 0;
    __syncthreads();
    if (tid < 3) {
        float l = FLT_MAX, h = -FLT_MAX;
        for (int w = 0; w < kWalkThreads / 64; ++w) { l = fminf(l, s_red[w][tid]); h = fmaxf(h, s_red[w][3 + tid]); }
        s_lo[tid] = l;
        s_scale[tid] = 16.0f / fmaxf(h - l, 1e-30f);          // (no finite coordinate on this axis: h - l < 0, every cell 0)
    }
    __syncthreads();

    // 2. histogram of the keys
    for (int i0 = tid; i0 < n; i0 += kWalkBatch * kWalkThreads) {
        walk_fetch(pts, i0, n, v);
#pragma unroll
        for (int u = 0; u < kWalkBatch; ++u) {
            const int i = i0 + u * kWalkThreads;
            if (i < n) {
                const int k = walk_key(v[u], s_lo, s_scale);
                atomicAdd(&s_bin[k], 1);
                if (key_out) key_out[i] = k;
            }
        }
    }
    __syncthreads();

    // 3. exclusive scan: four consecutive bins per thread
    int c[4], sum = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) { c[b] = s_bin[4 * tid + b]; sum += c[b]; }
    int total;
    int off = block_excl_scan_i32<kWalkThreads>(sum, &total, s_scan);
#pragma unroll
    for (int b = 0; b < 4; ++b) { s_bin[4 * tid + b] = off; off += c[b]; }
    __syncthreads();

    // 4. scatter through the bins' cursors.  Every cursor stays inside its bin, so every position is in [0, n) and is written
    // once: the keys are those of step 2 (same points, same box) and the bins' sizes are their counts.
    for (int i0 = tid; i0 < n; i0 += kWalkBatch * kWalkThreads) {
        walk_fetch(pts, i0, n, v);
#pragma unroll
        for (int u = 0; u < kWalkBatch; ++u) {
            const int i = i0 + u * kWalkThreads;
            if (i < n) {
                walk[atomicAdd(&s_bin[walk_key(v[u], s_lo, s_scale)], 1)] = i;
            }
        }
    }
}

}  // namespace

// walks of up to four clouds in one launch; key[g] may be NULL
int query_walk_multi(const float* const* pts, const int* n, int* const* walk, int* const* key, int count, hipStream_t st) {
    PCRCG_CHECK_ARG(pts && n && walk && count >= 1 && count <= 4);
    WalkMulti mm;
    int nmax = 0;
    for (int g = 0; g < 4; ++g) {
        const bool on = g < count;
        if (on) PCRCG_CHECK_ARG(n[g] >= 0 && (n[g] == 0 || (pts[g] && walk[g])));
        mm.pts[g] = on ? pts[g] : nullptr;
        mm.walk[g] = on ? walk[g] : nullptr;
        mm.key[g] = (on && key) ? key[g] : nullptr;
        mm.n[g] = on ? n[g] : 0;
        if (on && n[g] > nmax) nmax = n[g];
    }
    if (nmax == 0) return PCRCG_OK;
    hipLaunchKernelGGL(k_query_walk, dim3(count), dim3(kWalkThreads), 0, st, mm);
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}

}  // namespace pcrcg

using namespace pcrcg;

extern "C" {

int pcrcg_query_walk(const float* points, int n, int* walk, int* key, void* stream) {
    PCRCG_CHECK_ARG(n >= 0);
    if (n == 0) return PCRCG_OK;
    PCRCG_CHECK_ARG(points && walk);
    return query_walk_multi(&points, &n, &walk, key ? &key : nullptr, 1, as_stream(stream));
}

// the max-pool gather with the queries' order given: what the forward runner launches, for tests and A/B timing (the KPConv
// gather's _walk entries are in kpconv.hip)
int pcrcg_gather_max_walk(const float* x, int ns, int c, const int64_t* idx, int nq, int h, int ld_idx, float* out,
                          const int* walk, void* stream) {
    PCRCG_CHECK_ARG(ns >= 0 && c >= 1 && nq >= 0 && h >= 1 && ld_idx >= h);
    if (nq == 0) return PCRCG_OK;
    PCRCG_CHECK_ARG(x && idx && out);
    const GatherJob one{x, idx, out, ns, nq, h, ld_idx, walk};
    return gather_max_multi(&one, 1, c, as_stream(stream));
}
}
