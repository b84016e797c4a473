// chamfer.hip -- the modified Chamfer distance of the ModelNet evaluation for many ragged pairs (pcrcg_chamfer_batch;
// ref:lib/tester.py:280-286, compute_metrics).  Compiled without contraction (Makefile: EXACT_SRC): every product and sum
// below rounds on its own, as include/pcrcg.h states.
//
// Two brute-force nearest-neighbour searches per pair, both in ONE launch of k_chamfer_nn:
//   side 0: queries pred * points_src (moved once, by their lane)  candidates points_raw
//   side 1: queries points_ref                                     candidates (pred o gt^-1) * points_raw (moved while staged)
// One query per lane, held in registers; the candidates pass through LDS in tiles of kTile points as three planes, and
// every lane of the workgroup walks the same tile, so each LDS read is one address for the whole wavefront (a broadcast).
// Plain VALU work: per candidate and query 3 subtractions, 3 products, 2 sums (unfused) and the minimum -- 9 operations,
// 11 with the arg-min (compare + two selects instead of the minimum).
//
// Workgroups: 256 queries of ONE pair and side.  The grid is flat; pair b's query tiles of a side sit at the slots
// (off[b] >> 8) + b + k, k < ceil(n_b / 256) -- strictly increasing in b, at most (total >> 8) + B + 1 of them, so the
// host sizes the grid from the totals alone and a workgroup finds its pair by a binary search of the device offsets.  A
// slot that falls between two pairs leaves at once.  The same slot holds the workgroup's partial sum of minima (float64,
// added in a fixed tree order); k_chamfer_finish adds a pair's partials in slot order.  No floating-point atomics: a pair's
// results do not depend on B, on its position or on the schedule.
#include "common.h"

namespace pcrcg {
namespace {

constexpr int kTile = 1024;          // candidates per LDS tile: 3 planes x 4 KB
constexpr int kQ = 256;              // queries (= threads) per workgroup

struct ChamferArgs {
    const float* src; const int* src_off; int n_total;
    const float* ref; const int* ref_off; int m_total;
    const float* raw; const int* raw_off; int r_total;
    int B;
    const float* pred; const float* gt;
    float* d_src; int* arg_src; float* d_ref; int* arg_ref;
    double* part;                    // [slots_src + slots_ref]
    int slots_src, slots_ref;
};

__host__ __device__ inline int chamfer_slots(int total, int B) { return (total >> 8) + B + 1; }

// rows [o0, o0 + n) of pair b in a stack of `total` rows; an offset pair that does not describe a range inside the stack
// (a caller's mistake) reads as an empty cloud, so nothing is read out of bounds
__device__ inline void pair_range(const int* off, int b, int total, int& o0, int& n) {
    o0 = off[b];
    const int o1 = off[b + 1];
    n = o1 - o0;
    if (o0 < 0 || n < 0 || o1 > total) { o0 = 0; n = 0; }
}

// bit 0: a NaN coordinate; bits 1..3: +inf in x, y, z; bits 4..6: -inf in x, y, z.  A squared distance is NaN exactly when
// one of the two points has a NaN, or both have an infinity of the same sign in the same coordinate (inf - inf).
__device__ inline unsigned nonfinite_mask(float x, float y, float z) {
    const float inf = __builtin_inff();
    unsigned m = (x != x || y != y || z != z) ? 1u : 0u;
    m |= (x == inf ? 2u : 0u) | (y == inf ? 4u : 0u) | (z == inf ? 8u : 0u);
    m |= (x == -inf ? 16u : 0u) | (y == -inf ? 32u : 0u) | (z == -inf ? 64u : 0u);
    return m;
}

// pred o gt^-1 of one pair as R (row-major) then t, as the reference composes it: R = Rp Rg^T,
// t = Rp (-(Rg^T tg)) + tp, in float64 from the fp32 poses, rounded to fp32 once.  Entry e of 12.
__device__ inline float compose_entry(const float* P, const float* G, int e) {
    if (e < 9) {
        const int i = e / 3, j = e % 3;
        return (float)(((double)P[3 * i] * (double)G[3 * j] + (double)P[3 * i + 1] * (double)G[3 * j + 1]) +
                       (double)P[3 * i + 2] * (double)G[3 * j + 2]);
    }
    const int i = e - 9;
    double u[3];                     // -(Rg^T tg)
    for (int c = 0; c < 3; ++c)
        u[c] = -(((double)G[c] * (double)G[9] + (double)G[3 + c] * (double)G[10]) + (double)G[6 + c] * (double)G[11]);
    return (float)((((double)P[3 * i] * u[0] + (double)P[3 * i + 1] * u[1]) + (double)P[3 * i + 2] * u[2]) + (double)P[9 + i]);
}

template <bool ARG>
__global__ void __launch_bounds__(kQ) k_chamfer_nn(ChamferArgs s) {
    __shared__ __attribute__((aligned(16))) float cx[kTile], cy[kTile], cz[kTile];
    __shared__ float s_T[12];
    __shared__ int s_pair;
    __shared__ unsigned s_mask;
    __shared__ double s_wave[kQ / kWave];

    int g = blockIdx.x;
    const int side = g >= s.slots_src ? 1 : 0;
    if (side) g -= s.slots_src;
    const int* q_off = side ? s.ref_off : s.src_off;
    if (threadIdx.x == 0) {
        int lo = 0, hi = s.B - 1;    // the last pair whose first slot is <= g
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if ((q_off[mid] >> 8) + mid <= g) lo = mid; else hi = mid - 1;
        }
        s_pair = lo;
        s_mask = 0u;
    }
    __syncthreads();
    const int p = s_pair;
    int q0, nq, r0, nr;
    pair_range(q_off, p, side ? s.m_total : s.n_total, q0, nq);
    pair_range(s.raw_off, p, s.r_total, r0, nr);
    const int tile0 = g - ((q_off[p] >> 8) + p);
    if (tile0 < 0 || (long)tile0 * kQ >= nq) return;           // a slot between two pairs (the whole workgroup leaves)

    if (threadIdx.x < 12) {
        const float* P = s.pred + 12 * (long)p;
        s_T[threadIdx.x] = side ? compose_entry(P, s.gt + 12 * (long)p, threadIdx.x) : P[threadIdx.x];
    }
    __syncthreads();
    float T[12];
    for (int e = 0; e < 12; ++e) T[e] = s_T[e];

    const int i = tile0 * kQ + threadIdx.x;
    const bool live = i < nq;
    float x = 0.f, y = 0.f, z = 0.f;
    if (live) {
        const float* q = (side ? s.ref : s.src) + 3 * (long)(q0 + i);
        x = q[0]; y = q[1]; z = q[2];
        if (!side) {
            const float px = ((T[0] * x + T[1] * y) + T[2] * z) + T[9];
            const float py = ((T[3] * x + T[4] * y) + T[5] * z) + T[10];
            const float pz = ((T[6] * x + T[7] * y) + T[8] * z) + T[11];
            x = px; y = py; z = pz;
        }
    }
    const unsigned qmask = nonfinite_mask(x, y, z);

    float best = __builtin_inff();
    int arg = 0;
    const float* cand = s.raw + 3 * (long)r0;
    for (int t0 = 0; t0 < nr; t0 += kTile) {
        const int cnt = nr - t0 < kTile ? nr - t0 : kTile;
        const int cnt4 = (cnt + 3) & ~3;
        __syncthreads();                                        // the previous tile has been walked
        unsigned cm = 0u;
        for (int j = threadIdx.x; j < cnt4; j += kQ) {
            float a = __builtin_inff(), b = a, c = a;           // the tail of the last group of four: never the minimum
            if (j < cnt) {
                const float* r = cand + 3 * (long)(t0 + j);
                a = r[0]; b = r[1]; c = r[2];
                if (side) {
                    const float px = ((T[0] * a + T[1] * b) + T[2] * c) + T[9];
                    const float py = ((T[3] * a + T[4] * b) + T[5] * c) + T[10];
                    const float pz = ((T[6] * a + T[7] * b) + T[8] * c) + T[11];
                    a = px; b = py; c = pz;
                }
                cm |= nonfinite_mask(a, b, c);
            }
            cx[j] = a; cy[j] = b; cz[j] = c;
        }
        if (cm) atomicOr(&s_mask, cm);
        __syncthreads();
#pragma unroll 2
        for (int j = 0; j < cnt4; j += 4) {
            const float4 ax = *reinterpret_cast<const float4*>(&cx[j]);
            const float4 ay = *reinterpret_cast<const float4*>(&cy[j]);
            const float4 az = *reinterpret_cast<const float4*>(&cz[j]);
            const float vx[4] = {ax.x, ax.y, ax.z, ax.w}, vy[4] = {ay.x, ay.y, ay.z, ay.w}, vz[4] = {az.x, az.y, az.z, az.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float dx = x - vx[u], dy = y - vy[u], dz = z - vz[u];
                const float d = (dx * dx + dy * dy) + dz * dz;
                if (ARG) {
                    if (d < best) { best = d; arg = t0 + j + u; }   // ascending walk, strict: the lowest index on ties
                } else {
                    best = d < best ? d : best;
                }
            }
        }
    }
    __syncthreads();
    const unsigned cmask = s_mask;
    if (nr == 0 || (qmask & 1u) || (cmask & 1u) || (qmask & cmask & 0x7eu)) {   // no candidate, or a NaN distance in the row
        best = __builtin_nanf("");
        arg = -1;
    }
    if (live) {
        float* d_out = side ? s.d_ref : s.d_src;
        int* a_out = side ? s.arg_ref : s.arg_src;
        if (d_out) d_out[q0 + i] = best;
        if (ARG && a_out) a_out[q0 + i] = arg;
    }
    // the workgroup's sum of minima in float64: lanes by halving shuffles, the four wavefronts in order
    double v = live ? (double)best : 0.0;
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_down(v, o, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0) s_wave[threadIdx.x / kWave] = v;
    __syncthreads();
    if (threadIdx.x == 0) s.part[blockIdx.x] = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
}

// one thread per pair: its partials in slot order, the means, their sum
__global__ void __launch_bounds__(256) k_chamfer_finish(ChamferArgs s, float* __restrict__ chamfer, float* __restrict__ mean_src,
                                                        float* __restrict__ mean_ref) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= s.B) return;
    int o, n, m, r;
    pair_range(s.src_off, p, s.n_total, o, n);
    const int slot_s = (s.src_off[p] >> 8) + p;
    pair_range(s.ref_off, p, s.m_total, o, m);
    const int slot_r = s.slots_src + (s.ref_off[p] >> 8) + p;
    pair_range(s.raw_off, p, s.r_total, o, r);
    double ms = __builtin_nan(""), mr = ms;
    if (n > 0 && m > 0 && r > 0) {
        double a = 0.0, b = 0.0;
        for (int k = 0; k < (n + kQ - 1) / kQ; ++k) a += s.part[slot_s + k];
        for (int k = 0; k < (m + kQ - 1) / kQ; ++k) b += s.part[slot_r + k];
        ms = a / (double)n;
        mr = b / (double)m;
    }
    chamfer[p] = (float)(ms + mr);
    if (mean_src) mean_src[p] = (float)ms;
    if (mean_ref) mean_ref[p] = (float)mr;
}

constexpr int kMaxBatch = 65535;

}  // namespace
}  // namespace pcrcg

using namespace pcrcg;

extern "C" {

size_t pcrcg_chamfer_batch_ws_bytes(int B, int n_total, int m_total, int r_total) {
    if (B < 1 || B > kMaxBatch || n_total < 0 || m_total < 0 || r_total < 0) return 0;
    return carve_bytes((size_t)chamfer_slots(n_total, B) + (size_t)chamfer_slots(m_total, B), sizeof(double));
}

int pcrcg_chamfer_batch(const float* src, const int* src_off, int n_total, const float* ref, const int* ref_off, int m_total,
                        const float* raw, const int* raw_off, int r_total, int B, const float* pred, const float* gt,
                        float* chamfer, float* mean_src, float* mean_ref, float* d_src, int* arg_src, float* d_ref, int* arg_ref,
                        void* ws, size_t ws_bytes, void* stream) {
    PCRCG_CHECK_ARG(src && src_off && ref && ref_off && raw && raw_off && pred && gt && chamfer && ws);
    PCRCG_CHECK_ARG(B >= 1 && B <= kMaxBatch);
    PCRCG_CHECK_ARG(n_total >= 0 && m_total >= 0 && r_total >= 0);
    ChamferArgs a;
    a.slots_src = chamfer_slots(n_total, B);
    a.slots_ref = chamfer_slots(m_total, B);
    Carver cv(ws, ws_bytes);
    a.part = cv.take<double>((size_t)a.slots_src + (size_t)a.slots_ref);
    PCRCG_CHECK_WS(cv);
    a.src = src; a.src_off = src_off; a.n_total = n_total;
    a.ref = ref; a.ref_off = ref_off; a.m_total = m_total;
    a.raw = raw; a.raw_off = raw_off; a.r_total = r_total;
    a.B = B; a.pred = pred; a.gt = gt;
    a.d_src = d_src; a.arg_src = arg_src; a.d_ref = d_ref; a.arg_ref = arg_ref;
    hipStream_t st = as_stream(stream);
    const dim3 grid(a.slots_src + a.slots_ref);
    if (arg_src || arg_ref) hipLaunchKernelGGL(k_chamfer_nn<true>, grid, dim3(kQ), 0, st, a);
    else hipLaunchKernelGGL(k_chamfer_nn<false>, grid, dim3(kQ), 0, st, a);
    PCRCG_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_chamfer_finish, dim3((B + 255) / 256), dim3(256), 0, st, a, chamfer, mean_src, mean_ref);
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}

}  // extern "C"
