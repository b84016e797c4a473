// kpconv.hip -- KPConv neighbour gather + kernel-point aggregation on gfx950 (stage 1 of
// KPConv.forward, ref:models/blocks.py:264-354,369-372).  This is the dominant HBM-bound kernel of the
// path (bench.py `roofline`).
//
//   wf[q,k,c] = sum_h w[q,h,k] * x[idx[q,h],c],   w[q,h,k] = max(0, 1 - |s[idx[q,h]] - q - kp[k]| / extent)
//   n_q       = max(1, #{h : sum_c x[idx[q,h],c] > 0})                       (:369-371)
//
// Main kernel (k_kpconv_mfma): one wavefront per (query, channel chunk).  The aggregation is a
// [16 kernel points] x [H neighbours] x [channels] contraction, done on the matrix cores with
// v_mfma_f32_16x16x4_f32 (exact fp32).  Per step of 4 neighbours:
//   * lane (hsub = lane>>4, j = lane&15) evaluates ONE influence weight -- neighbour h0+hsub against
//     kernel point j -- which is exactly the A-operand element A[i=j][k=hsub] it must supply;
//   * the same lane loads one float4 of feature row idx[h0+hsub] at channel 4j: 16 lanes read a whole
//     256-byte row segment (coalesced), and the 4 components feed 4 MFMAs as B[k=hsub][col=j], so MFMA n
//     accumulates channels {4j+n};
//   * neighbour indices and centred neighbour coordinates are loaded once per 64 neighbours
//     (lanes = neighbours) and broadcast with wave shuffles; nothing is staged through LDS.
// The D layout (row = 4*(lane>>4)+r = kernel point, col = j) lets each lane store float4s of 4
// consecutive channels of wf.
// Shadow neighbours (idx == ns) have weight 0 and feature 0 in the reference (:269,:348): their weight
// is forced to 0 and no row is read.
//
// Fallbacks: k_kpconv_c1 for Cin == 1 (first layer, features are a column of ones; four lanes per query), and the scalar
// k_kpconv_generic for channel counts that are not a multiple of 4.
//
// Host side (kpconv.h): one descriptor, KpconvCall, and one entry, kpconv_run, for the fp32 gather, its bf16-storage form
// and the one-kernel first layer: it checks the call, carves the workspace (kpconv_ws), packs the support records if asked,
// plans (kpconv_plan) and launches.  Every C entry of the gather is in this file, the _walk ones included, and only fills a
// KpconvCall; so do the forward runner (runner.hip) and the transposed backward (transpose.hip).  wf is stored non-temporally
// in every form: it is streamed once through HBM and read back by the contraction.
#include <hip/hip_ext.h>

#include "kpconv.h"

namespace pcrcg {
namespace {

constexpr int K = PCRCG_KPOINTS;
constexpr int kWavesPerBlock = 4;
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned short bf16_rne(float f) {
    const unsigned u = __float_as_uint(f);
    return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// pos[s] = (sum_c x[s,c] > 0); one wavefront per support row.  Also writes the packed record
// pk[s] = (x, y, z, pos ? 1 : 0): the gather kernels fetch a neighbour's coordinates and flag with ONE 16-byte
// gather (one cache line) instead of a 12-byte and a 1-byte gather (two lines) -- random line fetches, not
// feature bytes, are what loads L2 in this kernel.
__global__ void __launch_bounds__(256) k_row_positive(const float* __restrict__ x, int ns, int cin,
                                                       const float* __restrict__ s_pts, unsigned char* __restrict__ pos,
                                                       float4* __restrict__ pk, unsigned short* __restrict__ xb) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= ns) return;
    float s = 0.0f;
    for (int c = lane; c < cin; c += 64) {
        const float v = x[(long)row * cin + c];
        s += v;
        if (xb) xb[(long)row * cin + c] = bf16_rne(v);      // bf16 feature-storage variant: the copy the gathers read
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    if (lane == 0) {
        pos[row] = s > 0.0f ? 1 : 0;
        pk[row] = make_float4(s_pts[3 * (long)row], s_pts[3 * (long)row + 1], s_pts[3 * (long)row + 2], s > 0.0f ? 1.f : 0.f);
    }
}

// Cin == 1: pk[s] = (x, y, z, feature)
__global__ void __launch_bounds__(256) k_pack_c1(const float* __restrict__ x, int ns, const float* __restrict__ s_pts,
                                                  float4* __restrict__ pk) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row < ns) pk[row] = make_float4(s_pts[3 * (long)row], s_pts[3 * (long)row + 1], s_pts[3 * (long)row + 2], x[row]);
}

struct __attribute__((packed, aligned(4))) P3 { float x, y, z; };

// BF16: the bf16 feature-storage variant (BASELINE.json configs[1] "bf16/fp32"): x and wf are bf16 in memory (half the
// gather and half the wf bytes), the aggregation still runs on the fp32 MFMA with fp32 accumulation; wf is rounded to
// nearest-even on the way out.
__device__ __forceinline__ float4 load4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 load4(const unsigned short* p) {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                       __uint_as_float(u.y & 0xffff0000u));
}

// TAIL (round 6, PCR-CG's 129-channel input in rows of 132 floats): cin = 64 NB + 4 with ONE wavefront per query -- the last
// float4 of a row does not get a 64-channel block of its own (a third wavefront per query that repeats the index loads,
// the shuffles and the 15 square roots for four channels: what the plain plan gave this width) but rides along on the vector
// units: every lane multiplies its influence weight with its neighbour's last float4 (the 16 lanes of a neighbour read one
// address), the four neighbour groups meet by two shuffles at the end.
template <int NB, typename FT, bool TAIL = false>  // 64-channel blocks handled per wavefront (one float4 per lane and block)
__global__ void __launch_bounds__(kWavesPerBlock * 64) k_kpconv_mfma(
    const float* __restrict__ q_pts, int nq, const float* __restrict__ s_pts, int ns,
    const long long* __restrict__ idx, int H, int ld_idx, const FT* __restrict__ x, int cin,
    const float* __restrict__ kp, float extent, const float4* __restrict__ pk, FT* __restrict__ wf,
    float* __restrict__ inv_n, int nchunk, const int* __restrict__ walk) {
    constexpr bool BF16 = sizeof(FT) == 2;
    // groups of 4 neighbours whose row reads are in flight together.  The kernel is bound by its dependent load
    // chain, so occupancy beats deeper batches: 4 groups (76 VGPRs, 6 wavefronts/SIMD) measured best for NB = 1
    // (8 groups: 96 VGPRs / 5 waves, -9 %; 12 groups: 136 / 3 waves, -40 %; 2 groups: 68 / 7 waves, -4 %)
    constexpr int STEPS = NB >= 4 ? 2 : 4;
    const int lane = threadIdx.x & 63;
    const int hsub = lane >> 4, j = lane & 15;
    // the wavefront index is uniform: telling the compiler so moves the item's query, its coordinates and the row
    // base addresses into SGPRs (fewer VGPRs -> more wavefronts per SIMD, which is what this kernel is short of)
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    long gw = (long)blockIdx.x * kWavesPerBlock + wave;
    long nw = (long)gridDim.x * kWavesPerBlock;
    long items = (long)nq * nchunk;
    // With a walk (walk.hip) the launch covers POSITIONS of the walk, q = walk[pos]: workgroup b runs on XCD b & 7, and XCD x
    // takes the x-th eighth of the positions (split as gemm_x6.hip splits its tiles), its workgroups striding through it
    // together -- the queries in flight on one XCD are a compact window of the Morton curve, so their neighbour rows meet in
    // that XCD's own L2.  The grid is a multiple of 8 workgroups then.  Without one: items in index order, as before.
    int pos0 = 0;
    if (walk) {
        const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, nslot = gridDim.x >> 3;
        const int xq = nq >> 3, xr = nq & 7;
        pos0 = xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq;
        gw = (long)slot * kWavesPerBlock + wave;
        nw = (long)nslot * kWavesPerBlock;
        // (readfirstlane: the compiler otherwise evaluates the select on the vector unit and keeps `items` in two VGPRs)
        const int cnt = __builtin_amdgcn_readfirstlane(xq + (xcd < xr ? 1 : 0));
        items = (long)cnt * nchunk;
    }
    const bool jvalid = j < K;
    const float kpx = jvalid ? kp[3 * j] : 0.f, kpy = jvalid ? kp[3 * j + 1] : 0.f, kpz = jvalid ? kp[3 * j + 2] : 0.f;
    const float inv_extent = 1.0f / extent;

    for (long item = gw; item < items; item += nw) {
        const int p = (int)(item / nchunk), chunk = (int)(item - (long)p * nchunk);
        int q = p;
        if (walk) {
            q = walk[pos0 + p];
            // The ONE guard against a corrupt walk: a walk is a permutation of 0 .. nq-1 (k_query_walk writes nothing else), and
            // an entry outside that range must not become an address outside the rows -- a stray store can take the device
            // down.  Such a walk gives duplicated and missing rows; the walk tests compare every row against index order.
            q = q < 0 ? 0 : (q < nq ? q : nq - 1);
        }
        const int c0 = chunk * 64 * NB;
        const float qx = q_pts[3 * (long)q], qy = q_pts[3 * (long)q + 1], qz = q_pts[3 * (long)q + 2];
        f32x4 acc[NB][4];
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[b][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
        int npos = 0;
        float ta0 = 0.f, ta1 = 0.f, ta2 = 0.f, ta3 = 0.f;             // TAIL: this lane's (kernel point j, neighbour group hsub) share
        for (int hc = 0; hc < H; hc += 64) {
            // lanes = neighbours: index + centred coordinates, once per 64 neighbours
            const int h = hc + lane;
            const long long iv = idx[(long)q * ld_idx + (h < H ? h : H - 1)];   // branch-free, clamped
            const int i = (h < H && iv >= 0 && iv < ns) ? (int)iv : -1;
            const long ic = i >= 0 ? i : 0;
            const float4 sp = pk[ic];                                      // coordinates + row-positive flag
            const float px = sp.x - qx, py = sp.y - qy, pz = sp.z - qz;
            if (chunk == 0) npos += __popcll(__ballot(i >= 0 && sp.w != 0.f));
            // the table pads a short row with shadow entries at its END: the groups behind the last real neighbour would
            // load (a clamped row), take 15 square roots and multiply by zero weights -- the loop stops at the last real one
            // (round 6; a row usually holds fewer neighbours than the table is wide: the limits sit at a high percentile)
            const unsigned long long real_lanes = __ballot(i >= 0);
            const int hn_all = H - hc < 64 ? H - hc : 64;
            const int hn_real = real_lanes ? 64 - (int)__clzll(real_lanes) : 0;
            const int hn = hn_real < hn_all ? hn_real : hn_all;
            // STEPS groups of 4 neighbours at a time: all their row reads are issued before the first
            // MFMA needs one (STEPS x NB KiB in flight per wavefront)
            for (int h0 = 0; h0 < hn; h0 += 4 * STEPS) {
                float w[STEPS];
                float4 v[STEPS][NB];
                float4 vt[STEPS];
#pragma unroll
                for (int s = 0; s < STEPS; ++s) {
                    const int src = h0 + 4 * s + hsub;            // <= 63
                    const int ii = __shfl(i, src, 64);
                    const float nx = __shfl(px, src, 64), ny = __shfl(py, src, 64), nz = __shfl(pz, src, 64);
                    const bool real = ii >= 0 && h0 + 4 * s < hn;
                    w[s] = 0.f;
                    if (real && jvalid) {
                        const float dx = nx - kpx, dy = ny - kpy, dz = nz - kpz;
                        w[s] = fmaxf(1.0f - __builtin_amdgcn_sqrtf(dx * dx + dy * dy + dz * dz) * inv_extent, 0.0f);
                    }
                    // unconditional loads from clamped (always valid) addresses, zeroed by select: a load
                    // inside a divergent branch would be waited for one by one
                    const FT* xrow = x + (long)(real ? ii : 0) * cin;
#pragma unroll
                    for (int b = 0; b < NB; ++b) {
                        const int c = c0 + 64 * b + 4 * j;
                        const float4 t = load4(xrow + (c < cin ? c : cin - 4));
                        const bool ok = real && c < cin;
                        v[s][b] = make_float4(ok ? t.x : 0.f, ok ? t.y : 0.f, ok ? t.z : 0.f, ok ? t.w : 0.f);
                    }
                    if constexpr (TAIL) {
                        const float4 t = load4(xrow + 64 * NB);
                        vt[s] = make_float4(real ? t.x : 0.f, real ? t.y : 0.f, real ? t.z : 0.f, real ? t.w : 0.f);
                    }
                }
#pragma unroll
                for (int s = 0; s < STEPS; ++s)
#pragma unroll
                    for (int b = 0; b < NB; ++b) {
                        acc[b][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[s], v[s][b].x, acc[b][0], 0, 0, 0);
                        acc[b][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[s], v[s][b].y, acc[b][1], 0, 0, 0);
                        acc[b][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[s], v[s][b].z, acc[b][2], 0, 0, 0);
                        acc[b][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[s], v[s][b].w, acc[b][3], 0, 0, 0);
                    }
                if constexpr (TAIL) {
#pragma unroll
                    for (int s = 0; s < STEPS; ++s) {
                        ta0 += w[s] * vt[s].x;
                        ta1 += w[s] * vt[s].y;
                        ta2 += w[s] * vt[s].z;
                        ta3 += w[s] * vt[s].w;
                    }
                }
            }
        }
        // D layout: register r of lane (hsub, j) = kernel point 4*hsub + r, channel group j
        FT* o = wf + (long)q * K * cin + c0;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const int c = 64 * b + 4 * j;
            if (c0 + c >= cin) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = 4 * hsub + r;
                if (k < K) {
                    // streamed once (the contraction GEMM reads it back): non-temporal, so that 230 MB of wf do not
                    // push the feature rows the gathers re-read out of L2
                    if constexpr (BF16) {
                        typedef unsigned v2u __attribute__((ext_vector_type(2)));
                        const v2u val = {(unsigned)bf16_rne(acc[b][0][r]) | ((unsigned)bf16_rne(acc[b][1][r]) << 16),
                                         (unsigned)bf16_rne(acc[b][2][r]) | ((unsigned)bf16_rne(acc[b][3][r]) << 16)};
                        __builtin_nontemporal_store(val, reinterpret_cast<v2u*>(o + (long)k * cin + c));
                    } else {
                        typedef float v4f __attribute__((ext_vector_type(4)));
                        const v4f val = {acc[b][0][r], acc[b][1][r], acc[b][2][r], acc[b][3][r]};
                        __builtin_nontemporal_store(val, reinterpret_cast<v4f*>(o + (long)k * cin + c));
                    }
                }
            }
        }
        if constexpr (TAIL) {
            ta0 += __shfl_xor(ta0, 16, 64); ta1 += __shfl_xor(ta1, 16, 64); ta2 += __shfl_xor(ta2, 16, 64); ta3 += __shfl_xor(ta3, 16, 64);
            ta0 += __shfl_xor(ta0, 32, 64); ta1 += __shfl_xor(ta1, 32, 64); ta2 += __shfl_xor(ta2, 32, 64); ta3 += __shfl_xor(ta3, 32, 64);
            if (hsub == 0 && jvalid) {
                typedef float v4f __attribute__((ext_vector_type(4)));
                const v4f val = {ta0, ta1, ta2, ta3};
                v4f* dst = reinterpret_cast<v4f*>(reinterpret_cast<float*>(wf) + (long)q * K * cin + (long)j * cin + 64 * NB);
                __builtin_nontemporal_store(val, dst);
            }
        }
        if (chunk == 0 && lane == 0) inv_n[q] = 1.0f / (float)(npos > 1 ? npos : 1);
    }
}

// Cin == 1 (first layer: the feature is a column of ones): wf[q,k] = sum_h w[q,h,k] * x[idx[q,h]].
// There is no channel dimension to spread over lanes and only Nq/64 wavefronts of thread-per-query work
// (fewer than the chip has SIMDs), so the kernel is bound by the idx -> coordinate load chain.  Four
// lanes share a query: each takes every fourth neighbour, C1_BATCH of them at a time with all index
// loads, then all gathers, in flight together; the 15 partial sums are combined with two butterfly
// shuffles.  Kernel points live in SGPRs, loads are branch-free (clamped addresses + select).
constexpr int C1_PARTS = 4, C1_BATCH = 6;
// The gather of one query by its four lanes (part = the lane's share of the neighbours): on return every lane holds the query's
// 15 influence sums and its count of neighbours with a positive feature.
__device__ __forceinline__ void c1_gather(const float* __restrict__ q_pts, int q, int part, int ns, const long long* __restrict__ idx,
                                          int H, int ld_idx, const float4* __restrict__ pk, const float* __restrict__ kp, float extent,
                                          float (&acc)[K], int& npos) {
    float kpx[K], kpy[K], kpz[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { kpx[k] = kp[3 * k]; kpy[k] = kp[3 * k + 1]; kpz[k] = kp[3 * k + 2]; }
    const float inv_extent = 1.0f / extent;
    const float qx = q_pts[3 * (long)q], qy = q_pts[3 * (long)q + 1], qz = q_pts[3 * (long)q + 2];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.f;
    npos = 0;
    const long long* row = idx + (long)q * ld_idx;
    for (int h0 = 0; h0 < H; h0 += C1_PARTS * C1_BATCH) {
        long long iv[C1_BATCH];
#pragma unroll
        for (int b = 0; b < C1_BATCH; ++b) {
            const int h = h0 + b * C1_PARTS + part;
            iv[b] = row[h < H ? h : H - 1];
        }
        float nx[C1_BATCH], ny[C1_BATCH], nz[C1_BATCH], xv[C1_BATCH];
#pragma unroll
        for (int b = 0; b < C1_BATCH; ++b) {
            const int h = h0 + b * C1_PARTS + part;
            const bool real = h < H && iv[b] >= 0 && iv[b] < ns;
            const long ic = real ? iv[b] : 0;
            const float4 p = pk[ic];                                     // one 16-byte gather: coordinates + feature
            nx[b] = p.x - qx;
            ny[b] = p.y - qy;
            nz[b] = p.z - qz;
            const float v = p.w;
            xv[b] = real ? v : 0.f;
        }
#pragma unroll
        for (int b = 0; b < C1_BATCH; ++b) {
            npos += xv[b] > 0.0f ? 1 : 0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float dx = nx[b] - kpx[k], dy = ny[b] - kpy[k], dz = nz[b] - kpz[k];
                acc[k] = fmaf(fmaxf(1.0f - __builtin_amdgcn_sqrtf(dx * dx + dy * dy + dz * dz) * inv_extent, 0.0f),
                              xv[b], acc[k]);
            }
        }
    }
#pragma unroll
    for (int d = 1; d < C1_PARTS; d <<= 1) {
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += __shfl_xor(acc[k], d, 64);
        npos += __shfl_xor(npos, d, 64);
    }
}

__global__ void __launch_bounds__(256) k_kpconv_c1(
    const float* __restrict__ q_pts, int nq, const float* __restrict__ s_pts, int ns,
    const long long* __restrict__ idx, int H, int ld_idx, const float4* __restrict__ pk, const float* __restrict__ kp,
    float extent, float* __restrict__ wf, float* __restrict__ inv_n, int ld_wf) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int part = t & (C1_PARTS - 1);
    const int qraw = t / C1_PARTS;
    const int q = qraw < nq ? qraw : nq - 1;          // surplus lanes shadow the last query (shuffles stay uniform)
    float acc[K];
    int npos;
    c1_gather(q_pts, q, part, ns, idx, H, ld_idx, pk, kp, extent, acc, npos);
    if (qraw >= nq) return;
#pragma unroll
    for (int k = 0; k < K; ++k)
        if ((k & (C1_PARTS - 1)) == part) wf[(long)q * ld_wf + k] = acc[k];
    if (ld_wf > K && part == C1_PARTS - 1) wf[(long)q * ld_wf + K] = 0.f;      // rows of 16 floats: the contraction's k-steps are whole
    if (part == 0) inv_n[q] = 1.0f / (float)(npos > 1 ? npos : 1);
}

// Cin == 1, the whole layer in one kernel: the gather of k_kpconv_c1 (the same loads, the same sums, the same n_q), then
//   y[q, c] = inv_n[q] * sum_k wf[q, k] * wt[c][k]        (fp64 FMAs, k = 0 .. 14 in order, ONE rounding to fp32)
// for the workgroup's 64 queries, and the column sums of the stored y for the InstanceNorm that follows -- no [nq, 16] wf
// matrix in memory and no K = 16 product through a kernel built for K in the hundreds.
// The contraction accumulates in fp64: y is then the correctly rounded product of the fp32 sums, as good as the split-term
// product it replaces (whose error on these shapes is the gather's own), where a chain of fifteen fp32 FMAs measured up to
// 2.6 times that product's error against float64 (tests/test_c1_fused_gpu.py allows 2).
// After the gather the roles turn: the 64 x 15 sums (and 1 / n_q) of the workgroup wait in LDS as doubles, a lane owns a
// COLUMN -- its 15 weights in registers, four 16-byte loads of its row of wt -- and wavefront w the queries 16 w .. 16 w + 15:
// a query costs a lane eight LDS reads that all lanes share and 15 FMAs, a wavefront's store is 256 contiguous bytes of one
// output row, and the lane sums its column as it goes: fp32 sums of the deviations from its first value, finished in fp64
// (the pivot form of the GEMM epilogue, gemm_x6.hip, whose lanes sum 16 rows as well).  The four wavefronts meet in LDS: ONE
// pair of fp64 atomics per column and 64-query tile -- the count that epilogue issues.  Widths above 64 take the columns in
// blocks of 64.  (First version: weights in LDS, lanes = queries, the output through an LDS tile: 42-49 KB of LDS kept a
// fifth of a 60 000-query launch's workgroups waiting for a CU, and the weight reads, one per FMA, ran at the LDS rate.)
constexpr int C1F_ROWS = 256 / C1_PARTS;          // queries per workgroup
__global__ void __launch_bounds__(256) k_kpconv_c1_fused(
    const float* __restrict__ q_pts, int nq, int ns, const long long* __restrict__ idx, int H, int ld_idx,
    const float4* __restrict__ pk, const float* __restrict__ kp, float extent, const float* __restrict__ wt, int cout,
    float* __restrict__ y, int ld_y, float* __restrict__ inv_n, double* __restrict__ sums) {
    __shared__ __attribute__((aligned(16))) double s_wf[C1F_ROWS][16];      // [query][k], [query][15] = 1 / n_q
    __shared__ double s_red[4][64][2];
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int part = t & (C1_PARTS - 1);
    const int qraw = t / C1_PARTS;
    const int q = qraw < nq ? qraw : nq - 1;          // surplus lanes shadow the last query (shuffles stay uniform)
    float acc[K];
    int npos;
    c1_gather(q_pts, q, part, ns, idx, H, ld_idx, pk, kp, extent, acc, npos);
    const float rn = 1.0f / (float)(npos > 1 ? npos : 1);
    if (qraw < nq && part == 0) inv_n[q] = rn;
    const int ql = threadIdx.x / C1_PARTS;
#pragma unroll
    for (int k = 0; k < K; ++k)
        if ((k & (C1_PARTS - 1)) == part) s_wf[ql][k] = (double)acc[k];
    if (part == C1_PARTS - 1) s_wf[ql][K] = (double)rn;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int q0 = blockIdx.x * C1F_ROWS;
    const int rows = nq - q0 < C1F_ROWS ? nq - q0 : C1F_ROWS;          // >= 1: the grid has no empty workgroup
    const int r0 = 16 * w, r1 = r0 + 16 < rows ? r0 + 16 : rows;
    for (int c0 = 0; c0 < cout; c0 += 64) {
        const int c = c0 + lane;
        double s = 0.0, s2 = 0.0;
        if (c < cout && r0 < rows) {
            double wd[16];
#pragma unroll
            for (int k4 = 0; k4 < 4; ++k4) {
                const float4 v = *reinterpret_cast<const float4*>(wt + (long)c * 16 + 4 * k4);
                wd[4 * k4] = (double)v.x; wd[4 * k4 + 1] = (double)v.y; wd[4 * k4 + 2] = (double)v.z; wd[4 * k4 + 3] = (double)v.w;
            }
            float piv = 0.f, cs = 0.f, cq = 0.f;
            for (int r = r0; r < r1; ++r) {
                double o = 0.0;
#pragma unroll
                for (int k = 0; k < K; ++k) o = fma(s_wf[r][k], wd[k], o);
                const float v = (float)(o * s_wf[r][K]);
                y[(long)(q0 + r) * ld_y + c] = v;
                if (r == r0) piv = v;
                const float d = v - piv;
                cs += d;
                cq += d * d;
            }
            const double p = (double)piv, s1 = (double)cs, n = (double)(r1 - r0);
            s = s1 + n * p;
            s2 = (double)cq + p * (2.0 * s1 + n * p);
        }
        s_red[w][lane][0] = s;
        s_red[w][lane][1] = s2;
        __syncthreads();
        if (w == 0 && c < cout) {
            unsafeAtomicAdd(&sums[c], (s_red[0][lane][0] + s_red[1][lane][0]) + (s_red[2][lane][0] + s_red[3][lane][0]));
            unsafeAtomicAdd(&sums[cout + c], (s_red[0][lane][1] + s_red[1][lane][1]) + (s_red[2][lane][1] + s_red[3][lane][1]));
        }
        __syncthreads();                                   // s_red is free for the next 64 columns
    }
}

// Scalar fallback for channel counts that are not a multiple of 4: weights staged in LDS, lanes =
// channels.
__global__ void __launch_bounds__(kWavesPerBlock * 64) k_kpconv_generic(
    const float* __restrict__ q_pts, int nq, const float* __restrict__ s_pts, int ns,
    const long long* __restrict__ idx, int H, int ld_idx, const float* __restrict__ x, int cin,
    const float* __restrict__ kp, float extent, const unsigned char* __restrict__ pos, float* __restrict__ wf,
    float* __restrict__ inv_n) {
    __shared__ __attribute__((aligned(16))) float s_w[kWavesPerBlock][64][16];
    __shared__ int s_idx[kWavesPerBlock][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gw = blockIdx.x * kWavesPerBlock + wave, nw = gridDim.x * kWavesPerBlock;
    const float inv_extent = 1.0f / extent;
    for (int q = gw; q < nq; q += nw) {
        const float qx = q_pts[3 * (long)q], qy = q_pts[3 * (long)q + 1], qz = q_pts[3 * (long)q + 2];
        int npos = 0;
        for (int cbase = 0; cbase < cin; cbase += 64) {
            float acc[K];
#pragma unroll
            for (int k = 0; k < K; ++k) acc[k] = 0.0f;
            for (int hc = 0; hc < H; hc += 64) {
                const int h = hc + lane;
                int i = -1;
                if (h < H) {
                    const long long v = idx[(long)q * ld_idx + h];
                    i = (v >= 0 && v < ns) ? (int)v : -1;
                }
                __builtin_amdgcn_wave_barrier();
                if (i >= 0) {
                    const float nx = s_pts[3 * (long)i] - qx, ny = s_pts[3 * (long)i + 1] - qy,
                                nz = s_pts[3 * (long)i + 2] - qz;
                    for (int k = 0; k < K; ++k) {
                        const float dx = nx - kp[3 * k], dy = ny - kp[3 * k + 1], dz = nz - kp[3 * k + 2];
                        s_w[wave][lane][k] = fmaxf(1.0f - sqrtf(dx * dx + dy * dy + dz * dz) * inv_extent, 0.0f);
                    }
                }
                s_idx[wave][lane] = i;
                if (cbase == 0) npos += __popcll(__ballot(i >= 0 && pos[i >= 0 ? i : 0] != 0));
                __builtin_amdgcn_wave_barrier();
                const int hn = H - hc < 64 ? H - hc : 64;
                const int c = cbase + lane;
                for (int hh = 0; hh < hn; ++hh) {
                    const int ii = s_idx[wave][hh];
                    if (ii < 0) continue;
                    const float xv = c < cin ? x[(long)ii * cin + c] : 0.0f;
#pragma unroll
                    for (int k = 0; k < K; ++k) acc[k] = fmaf(s_w[wave][hh][k], xv, acc[k]);
                }
            }
            const int c = cbase + lane;
            if (c < cin)
#pragma unroll
                for (int k = 0; k < K; ++k) wf[(long)q * K * cin + (long)k * cin + c] = acc[k];
        }
        if (lane == 0) inv_n[q] = 1.0f / (float)(npos > 1 ? npos : 1);
    }
}

}  // namespace

int kpconv_ws(void* ws, size_t ws_bytes, int ns, KpWs* out) {
    Carver cv(ws, ws_bytes);
    out->pos = cv.take<unsigned char>((size_t)ns + 1);
    out->pk = cv.take<float4>((size_t)ns + 1);
    PCRCG_CHECK_WS(cv);
    return PCRCG_OK;
}

int kpconv_pack(const float* x, int ns, int cin, const float* s_pts, const KpWs& w, hipStream_t st, unsigned short* x_bf16) {
    if (ns > 0) hipLaunchKernelGGL(k_row_positive, dim3((ns + 3) / 4), dim3(256), 0, st, x, ns, cin, s_pts, w.pos, w.pk, x_bf16);
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}

// widths of whole float4s, and weight rows a lane can read as four
bool kpconv_c1_fused_ok(int cout, const float* wt) { return cout >= 4 && cout % 4 == 0 && wt && (reinterpret_cast<uintptr_t>(wt) & 15) == 0; }

int kpconv_run(const KpconvCall& c) {
    const bool bf16 = c.form == KpForm::bf16, fused = c.form == KpForm::c1_fused;
    const int nq = c.nq, ns = c.ns, h = c.h, cin = fused ? 1 : c.cin;
    // everything that is refused for an empty call as well (the forms differ: tests/test_kpconv_args_cpu.py)
    PCRCG_CHECK_ARG(nq >= 0 && ns >= 0 && h >= 1 && c.ld_idx >= h && cin >= 1 && c.extent > 0.0f);
    if (bf16) PCRCG_CHECK_ARG(ns >= 1 && cin % 4 == 0);
    else if (fused) PCRCG_CHECK_ARG(kpconv_c1_fused_ok(c.cout, c.wt) && c.ld_y >= c.cout);
    else PCRCG_CHECK_ARG(c.c1_ld == 0 || c.c1_ld == K || c.c1_ld == K + 1);
    if (nq == 0) return PCRCG_OK;
    PCRCG_CHECK_ARG(c.q_pts && c.s_pts && c.idx && c.x && c.kp && c.inv_n && c.ws && ns >= 1);
    if (bf16)
        PCRCG_CHECK_ARG(c.x_bf16 && c.wf_bf16 && (reinterpret_cast<uintptr_t>(c.x_bf16) & 7) == 0 &&
                        (reinterpret_cast<uintptr_t>(c.wf_bf16) & 7) == 0);
    else if (fused) PCRCG_CHECK_ARG(c.y && c.sums);
    else PCRCG_CHECK_ARG(c.wf);
    KpWs w;
    PCRCG_PROPAGATE(kpconv_ws(c.ws, c.ws_bytes, ns, &w));
    const long long* idx_ll = reinterpret_cast<const long long*>(c.idx);
    if (cin == 1) {
        if (c.pack) hipLaunchKernelGGL(k_pack_c1, dim3((ns + 255) / 256), dim3(256), 0, c.st, c.x, ns, c.s_pts, w.pk);
    } else if (c.pack) {
        PCRCG_PROPAGATE(kpconv_pack(c.x, ns, cin, c.s_pts, w, c.st, bf16 ? c.x_bf16 : nullptr));
    }
    // start / stop events of the gather kernel itself; kind 1: the one-kernel layer, 2: bf16 storage
    KpProfScope prof(c.st, nq, h, cin, fused ? c.cout : 0, fused ? 1 : bf16 ? 2 : 0);
    const dim3 c1_grid((int)(((long)nq * C1_PARTS + 255) / 256));
    if (fused) {
        hipExtLaunchKernelGGL(k_kpconv_c1_fused, c1_grid, dim3(256), 0, c.st, prof.a, prof.b, 0, c.q_pts, nq, ns, idx_ll, h,
                              c.ld_idx, (const float4*)w.pk, c.kp, c.extent, c.wt, c.cout, c.y, c.ld_y, c.inv_n, c.sums);
    } else if (cin == 1) {
        hipExtLaunchKernelGGL(k_kpconv_c1, c1_grid, dim3(256), 0, c.st, prof.a, prof.b, 0, c.q_pts, nq, c.s_pts, ns, idx_ll, h,
                              c.ld_idx, (const float4*)w.pk, c.kp, c.extent, c.wf, c.inv_n, c.c1_ld > 0 ? c.c1_ld : K);
    } else if (!bf16 && !kpconv_vec_ok(cin, c.x, c.wf)) {
        hipLaunchKernelGGL(k_kpconv_generic, dim3(kpconv_blocks(nq)), dim3(kWavesPerBlock * 64), 0, c.st, c.q_pts, nq, c.s_pts,
                           ns, idx_ll, h, c.ld_idx, c.x, cin, c.kp, c.extent, (const unsigned char*)w.pos, c.wf, c.inv_n);
    } else {
        const KpPlan p = kpconv_plan(nq, cin, c.walk != nullptr, !bf16);
#define LAUNCH(NBV, FT, TAILV, X, WF)                                                                                          \
        hipExtLaunchKernelGGL((k_kpconv_mfma<NBV, FT, TAILV>), dim3(p.blocks), dim3(kWavesPerBlock * 64), 0, c.st, prof.a,    \
                              prof.b, 0, c.q_pts, nq, c.s_pts, ns, idx_ll, h, c.ld_idx, X, cin, c.kp, c.extent,               \
                              (const float4*)w.pk, WF, c.inv_n, p.nchunk, c.walk)
        if (bf16) {
            if (p.nb == 4) LAUNCH(4, unsigned short, false, c.x_bf16, c.wf_bf16);
            else if (p.nb == 2) LAUNCH(2, unsigned short, false, c.x_bf16, c.wf_bf16);
            else LAUNCH(1, unsigned short, false, c.x_bf16, c.wf_bf16);
        } else if (p.tail) {
            if (p.nb == 2) LAUNCH(2, float, true, c.x, c.wf);
            else LAUNCH(1, float, true, c.x, c.wf);
        } else {
            if (p.nb == 4) LAUNCH(4, float, false, c.x, c.wf);
            else if (p.nb == 2) LAUNCH(2, float, false, c.x, c.wf);
            else LAUNCH(1, float, false, c.x, c.wf);
        }
#undef LAUNCH
    }
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}

}  // namespace pcrcg

using namespace pcrcg;

// what every C entry of the gather passes on as it got it
static KpconvCall entry_call(const float* q_pts, int nq, const float* s_pts, int ns, const int64_t* idx, int h, int ld_idx,
                             const float* x, int cin, const float* kp, float extent, float* inv_n, void* ws, size_t ws_bytes,
                             const int* walk, void* stream) {
    KpconvCall c;
    c.q_pts = q_pts; c.nq = nq; c.s_pts = s_pts; c.ns = ns;
    c.idx = idx; c.h = h; c.ld_idx = ld_idx;
    c.x = x; c.cin = cin; c.kp = kp; c.extent = extent;
    c.inv_n = inv_n; c.ws = ws; c.ws_bytes = ws_bytes;
    c.walk = walk; c.st = as_stream(stream);
    return c;
}

extern "C" {

size_t pcrcg_kpconv_ws_bytes(int ns) {
    const size_t n = (size_t)(ns > 0 ? ns : 0) + 1;
    return carve_bytes(n, 1) + carve_bytes(n, sizeof(float4));     // row-positive flags + packed (x, y, z, flag) records
}

// the _walk entries: the queries' order given -- what the forward runner launches, for tests and A/B timing
int pcrcg_kpconv_aggregate_walk(const float* q_pts, int nq, const float* s_pts, int ns, const int64_t* idx, int h, int ld_idx,
                                const float* x, int cin, const float* kp, float extent, float* wf, float* inv_n, void* ws,
                                size_t ws_bytes, const int* walk, void* stream) {
    KpconvCall c = entry_call(q_pts, nq, s_pts, ns, idx, h, ld_idx, x, cin, kp, extent, inv_n, ws, ws_bytes, walk, stream);
    c.wf = wf;
    return kpconv_run(c);
}

int pcrcg_kpconv_aggregate(const float* q_pts, int nq, const float* s_pts, int ns, const int64_t* idx, int h, int ld_idx,
                           const float* x, int cin, const float* kp, float extent, float* wf, float* inv_n, void* ws,
                           size_t ws_bytes, void* stream) {
    return pcrcg_kpconv_aggregate_walk(q_pts, nq, s_pts, ns, idx, h, ld_idx, x, cin, kp, extent, wf, inv_n, ws, ws_bytes, nullptr,
                                       stream);
}

// The bf16 feature-storage variant of pcrcg_kpconv_aggregate: x stays fp32 at the boundary (the support-record prelude reads
// it: the n_q normaliser counts rows with a positive fp32 sum, exactly as the fp32 path does); `x_bf16` ([ns, cin] u16
// scratch) receives its round-to-nearest-even copy, which is what the neighbour gathers read, and `wf_bf16`
// ([nq, 15*cin] u16) the aggregated features rounded the same way.  Geometry, influences, the neighbour-count
// normaliser and the accumulation are fp32 as in the fp32 path.
int pcrcg_kpconv_aggregate_bf16_walk(const float* q_pts, int nq, const float* s_pts, int ns, const int64_t* idx, int h,
                                     int ld_idx, const float* x, int cin, const float* kp, float extent, void* x_bf16,
                                     void* wf_bf16, float* inv_n, void* ws, size_t ws_bytes, const int* walk, void* stream) {
    KpconvCall c = entry_call(q_pts, nq, s_pts, ns, idx, h, ld_idx, x, cin, kp, extent, inv_n, ws, ws_bytes, walk, stream);
    c.form = KpForm::bf16;
    c.x_bf16 = static_cast<unsigned short*>(x_bf16);
    c.wf_bf16 = static_cast<unsigned short*>(wf_bf16);
    return kpconv_run(c);
}

int pcrcg_kpconv_aggregate_bf16(const float* q_pts, int nq, const float* s_pts, int ns, const int64_t* idx, int h,
                                int ld_idx, const float* x, int cin, const float* kp, float extent, void* x_bf16,
                                void* wf_bf16, float* inv_n, void* ws, size_t ws_bytes, void* stream) {
    return pcrcg_kpconv_aggregate_bf16_walk(q_pts, nq, s_pts, ns, idx, h, ld_idx, x, cin, kp, extent, x_bf16, wf_bf16, inv_n, ws,
                                            ws_bytes, nullptr, stream);
}

int pcrcg_kpconv_c1_layer(const float* q_pts, int nq, const float* s_pts, int ns, const int64_t* idx, int h, int ld_idx,
                          const float* x, const float* kp, float extent, const float* wt, int cout, float* out, int ld_out,
                          float* inv_n, void* sums, void* ws, size_t ws_bytes, void* stream) {
    KpconvCall c = entry_call(q_pts, nq, s_pts, ns, idx, h, ld_idx, x, 1, kp, extent, inv_n, ws, ws_bytes, nullptr, stream);
    c.form = KpForm::c1_fused;
    c.wt = wt; c.cout = cout; c.y = out; c.ld_y = ld_out;
    c.sums = static_cast<double*>(sums);
    return kpconv_run(c);
}
}
