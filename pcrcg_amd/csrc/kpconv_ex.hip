// kpconv_ex.hip -- the general KPConv gather: deformable and modulated kernels, every influence function and both
// aggregation modes of ref:models/blocks.py:229-374 (stage 1 of KPConv.forward; stage 2 is the same wf @ W contraction
// as for the rigid kernel).  kpconv.hip keeps the rigid / linear / sum configuration of the shipped architectures; this
// file serves everything else and is built with contraction off (the deformed kernel points are offset * extent + kp,
// a product and a sum, as the reference rounds them).
//
//   kp_q[k]   = offset_features[q, 3k..3k+2] * extent + kp[k]                     (rigid: kp[k])          (:258,279)
//   d2[q,h,k] = |s[idx[q,h]] - q - kp_q[k]|^2          (shadow idx == ns: the point (1e6, 1e6, 1e6))      (:269-289)
//   kept(q,h) = deformable ? any_k d2 < extent^2 : true                                                  (:292-316)
//   w[q,h,k]  = constant 1 | linear max(0, 1 - sqrt(d2) / extent) | gaussian exp(-d2 / (2 (0.3 extent)^2 + 1e-9));
//               closest: only k* = argmin_k d2 (first index on ties) keeps its weight                     (:321-342)
//   wf[q,k,:] = sum_{h kept} w * x[idx[q,h],:]   (* 2 sigmoid(offset_features[q, 3K+k]) when modulated)   (:354-358)
//   n_q       = max(1, #{h kept : sum_c x[idx[q,h],c] > 0})                                              (:369-372)
//   min_d2[q,k] = min over ALL h < H of d2, shadow columns included                                       (:295)
//
// k_kpconv_ex_mfma follows the plan of k_kpconv_mfma (kpconv.hip): one wavefront per (query, channel chunk), lane
// (hsub = lane >> 4, j = lane & 15) evaluates neighbour h0 + hsub against kernel point j and supplies that weight as
// the A element of v_mfma_f32_16x16x4_f32; the 16 lanes of a neighbour read one 256-byte segment of its feature row.
// What is new: the kernel points are the item's own (lane j holds kp_q[j]); the kept bit of a neighbour is the OR over
// its 16 lanes (one ballot per step); closest mode is a 16-lane (d2, k) argmin by four butterfly shuffles; min_d2 is a
// running per-lane minimum, joined over the four neighbour groups at the end.  A neighbour that is not kept reads no
// feature row of its own (its address is clamped to row 0, as a shadow's is, and the value discarded).
// k_kpconv_ex_scalar (cin == 1, channel counts that are no multiple of 4, unaligned rows) is a plain restatement:
// one wavefront per query, lanes = channels, neighbours in turn.
// The backward (pcrcg_kpconv_backward_ex: dx and the gradient of offset_features) follows the forward entry in this file,
// so that both are built with the same flags and decide the kept bit and the argmin by the same expressions: the deformed
// kernel point, the modulation and the argmin's tie rule are device functions all four kernels call (deformed, modulation,
// argmin_takes).  The host side shares kpconv.h with kpconv.hip -- the workspace layout (kpconv_ws), the pack, the channel
// plan (kpconv_plan, never a tail, never a walk) and kpconv_vec_ok -- but keeps its own launches: it does not go through
// kpconv_run.  Both entries take their common argument checks from ex_check.
#include <hip/hip_ext.h>

#include "kpconv.h"
#include "pcrcg_train.h"
#include "scatter.h"

namespace pcrcg {
namespace {

constexpr int K = PCRCG_KPOINTS;
constexpr int kWavesPerBlock = 4;
constexpr float kShadow = 1e6f;
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct ExMode {
    int influence;      // 0 constant, 1 linear, 2 gaussian
    int closest, modulated;
    float extent, ext2, gauss_den;
};

__device__ __forceinline__ float influence_of(float d2, const ExMode& m) {
    if (m.influence == 0) return 1.0f;
    if (m.influence == 1) return fmaxf(1.0f - sqrtf(d2) / m.extent, 0.0f);
    return expf(-d2 / m.gauss_den);
}

// The expressions the four kernels must agree on, bit for bit.
// one coordinate of a deformed kernel point: a product and a sum, as the reference rounds them (contraction is off)
__device__ __forceinline__ float deformed(float o, float extent, float kp) { return o * extent + kp; }
// m = 2 sigmoid(off[q, 3K + k])
__device__ __forceinline__ float modulation(const float* off, long q, int ld_off, int k) {
    return 2.0f * (1.0f / (1.0f + expf(-off[q * ld_off + 3 * K + k])));
}
// butterfly argmin over (d2, k): the smaller distance, the smaller index on ties
__device__ __forceinline__ bool argmin_takes(float od, int ok, float bd, int bk) { return od < bd || (od == bd && ok < bk); }

template <int NB>
__global__ void __launch_bounds__(kWavesPerBlock * 64) k_kpconv_ex_mfma(
    const float* __restrict__ q_pts, int nq, int ns, const long long* __restrict__ idx, int H, int ld_idx,
    const float* __restrict__ x, int cin, const float* __restrict__ kp, const float* __restrict__ off, int ld_off,
    ExMode mode, const float4* __restrict__ pk, float* __restrict__ wf, float* __restrict__ inv_n,
    float* __restrict__ min_d2, int nchunk) {
    constexpr int STEPS = NB >= 4 ? 2 : 4;
    const int lane = threadIdx.x & 63;
    const int hsub = lane >> 4, j = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long gw = (long)blockIdx.x * kWavesPerBlock + wave;
    const long nw = (long)gridDim.x * kWavesPerBlock;
    const long items = (long)nq * nchunk;
    const bool jvalid = j < K;
    const float kx0 = jvalid ? kp[3 * j] : 0.f, ky0 = jvalid ? kp[3 * j + 1] : 0.f, kz0 = jvalid ? kp[3 * j + 2] : 0.f;
    const bool deform = off != nullptr;

    for (long item = gw; item < items; item += nw) {
        const int q = (int)(item / nchunk), chunk = (int)(item - (long)q * nchunk);
        const int c0 = chunk * 64 * NB;
        const float qx = q_pts[3 * (long)q], qy = q_pts[3 * (long)q + 1], qz = q_pts[3 * (long)q + 2];
        float kpx = kx0, kpy = ky0, kpz = kz0;
        if (deform && jvalid) {
            const float* o = off + (long)q * ld_off + 3 * j;
            kpx = deformed(o[0], mode.extent, kx0);
            kpy = deformed(o[1], mode.extent, ky0);
            kpz = deformed(o[2], mode.extent, kz0);
        }
        const bool want_min = min_d2 != nullptr && chunk == 0;
        f32x4 acc[NB][4];
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[b][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
        int npos = 0;
        float dmin = INFINITY;
        bool any_shadow = false;
        for (int hc = 0; hc < H; hc += 64) {
            // lanes = neighbours: index, centred coordinates and row-positive flag, once per 64 neighbours
            const int h = hc + lane;
            const long long iv = idx[(long)q * ld_idx + (h < H ? h : H - 1)];
            const int i = (h < H && iv >= 0 && iv < ns) ? (int)iv : -1;
            const float4 sp = pk[i >= 0 ? i : 0];
            const float px = sp.x - qx, py = sp.y - qy, pz = sp.z - qz;
            const bool pos = i >= 0 && sp.w != 0.f;
            any_shadow = any_shadow || __ballot(h < H && i < 0) != 0ull;
            const unsigned long long real_lanes = __ballot(i >= 0);
            const int hn = real_lanes ? 64 - (int)__clzll(real_lanes) : 0;      // behind the last real neighbour: shadows only
            for (int h0 = 0; h0 < hn; h0 += 4 * STEPS) {
                float w[STEPS];
                float4 v[STEPS][NB];
#pragma unroll
                for (int s = 0; s < STEPS; ++s) {
                    const int src = (h0 + 4 * s + hsub) & 63;
                    const int ii = __shfl(i, src, 64);
                    const float nx = __shfl(px, src, 64), ny = __shfl(py, src, 64), nz = __shfl(pz, src, 64);
                    const int pp = __shfl((int)pos, src, 64);
                    const bool real = ii >= 0 && h0 + 4 * s + hsub < hn;
                    const float dx = nx - kpx, dy = ny - kpy, dz = nz - kpz;
                    const float d2 = (real && jvalid) ? dx * dx + dy * dy + dz * dz : INFINITY;
                    dmin = fminf(dmin, d2);
                    // kept: any of the neighbour's 16 lanes in range (rigid: every real neighbour)
                    bool kept = real;
                    if (deform) {
                        const unsigned long long inr = __ballot(d2 < mode.ext2);
                        kept = ((inr >> (16 * hsub)) & 0xffffull) != 0ull;
                    }
                    float wv = influence_of(d2 == INFINITY ? 0.f : d2, mode);
                    if (mode.closest) {
                        float bd = d2;
                        int bk = j;
#pragma unroll
                        for (int m = 1; m < 16; m <<= 1) {
                            const float od = __shfl_xor(bd, m, 64);
                            const int ok = __shfl_xor(bk, m, 64);
                            const bool take = argmin_takes(od, ok, bd, bk);
                            bd = take ? od : bd;
                            bk = take ? ok : bk;
                        }
                        if (bk != j) wv = 0.f;
                    }
                    w[s] = (kept && jvalid) ? wv : 0.f;
                    if (chunk == 0 && j == 0 && kept && pp) ++npos;
                    const float* xrow = x + (long)(kept ? ii : 0) * cin;
#pragma unroll
                    for (int b = 0; b < NB; ++b) {
                        const int c = c0 + 64 * b + 4 * j;
                        const float4 t = *reinterpret_cast<const float4*>(xrow + (c < cin ? c : cin - 4));
                        const bool ok = kept && c < cin;
                        v[s][b] = make_float4(ok ? t.x : 0.f, ok ? t.y : 0.f, ok ? t.z : 0.f, ok ? t.w : 0.f);
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
            }
        }
        // D layout: register r of lane (hsub, j) = kernel point 4*hsub + r, channel group j
        float mod[4] = {1.f, 1.f, 1.f, 1.f};
        if (mode.modulated) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = 4 * hsub + r;
                if (k < K) mod[r] = modulation(off, q, ld_off, k);
            }
        }
        float* o = wf + (long)q * K * cin + c0;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const int c = 64 * b + 4 * j;
            if (c0 + c >= cin) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = 4 * hsub + r;
                if (k < K) {
                    typedef float v4f __attribute__((ext_vector_type(4)));
                    const v4f val = {acc[b][0][r] * mod[r], acc[b][1][r] * mod[r], acc[b][2][r] * mod[r], acc[b][3][r] * mod[r]};
                    __builtin_nontemporal_store(val, reinterpret_cast<v4f*>(o + (long)k * cin + c));
                }
            }
        }
        if (chunk == 0) {
            npos += __shfl_xor(npos, 16, 64);
            npos += __shfl_xor(npos, 32, 64);
            if (lane == 0) inv_n[q] = 1.0f / (float)(npos > 1 ? npos : 1);
        }
        if (want_min) {
            dmin = fminf(dmin, __shfl_xor(dmin, 16, 64));
            dmin = fminf(dmin, __shfl_xor(dmin, 32, 64));
            if (any_shadow) {       // every shadow column is the same point
                const float dx = (kShadow - qx) - kpx, dy = (kShadow - qy) - kpy, dz = (kShadow - qz) - kpz;
                dmin = fminf(dmin, dx * dx + dy * dy + dz * dz);
            }
            if (hsub == 0 && jvalid) min_d2[(long)q * K + j] = dmin;
        }
    }
}

// Plain restatement for cin == 1, channel counts that are no multiple of 4 and unaligned rows: one wavefront per query,
// lanes = channels, neighbours in turn; every lane evaluates the neighbour's 15 distances itself.
__global__ void __launch_bounds__(kWavesPerBlock * 64) k_kpconv_ex_scalar(
    const float* __restrict__ q_pts, int nq, const float* __restrict__ s_pts, int ns, const long long* __restrict__ idx, int H,
    int ld_idx, const float* __restrict__ x, int cin, const float* __restrict__ kp, const float* __restrict__ off, int ld_off,
    ExMode mode, const unsigned char* __restrict__ pos, float* __restrict__ wf, float* __restrict__ inv_n,
    float* __restrict__ min_d2) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gw = blockIdx.x * kWavesPerBlock + wave, nw = gridDim.x * kWavesPerBlock;
    for (int q = gw; q < nq; q += nw) {
        const float qx = q_pts[3 * (long)q], qy = q_pts[3 * (long)q + 1], qz = q_pts[3 * (long)q + 2];
        float kpx[K], kpy[K], kpz[K], mod[K], dmin[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            kpx[k] = kp[3 * k]; kpy[k] = kp[3 * k + 1]; kpz[k] = kp[3 * k + 2];
            if (off) {
                const float* o = off + (long)q * ld_off + 3 * k;
                kpx[k] = deformed(o[0], mode.extent, kpx[k]);
                kpy[k] = deformed(o[1], mode.extent, kpy[k]);
                kpz[k] = deformed(o[2], mode.extent, kpz[k]);
            }
            mod[k] = mode.modulated ? modulation(off, q, ld_off, k) : 1.0f;
            dmin[k] = INFINITY;
        }
        int npos = 0;
        for (int cbase = 0; cbase < cin; cbase += 64) {
            const int c = cbase + lane;
            float acc[K];
#pragma unroll
            for (int k = 0; k < K; ++k) acc[k] = 0.0f;
            for (int h = 0; h < H; ++h) {
                const long long iv = idx[(long)q * ld_idx + h];
                const bool real = iv >= 0 && iv < ns;
                const long i = real ? (long)iv : 0;
                const float nx = (real ? s_pts[3 * i] : kShadow) - qx, ny = (real ? s_pts[3 * i + 1] : kShadow) - qy,
                            nz = (real ? s_pts[3 * i + 2] : kShadow) - qz;
                float d2[K];
                bool inr = false;
                int kmin = 0;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const float dx = nx - kpx[k], dy = ny - kpy[k], dz = nz - kpz[k];
                    d2[k] = dx * dx + dy * dy + dz * dz;
                    inr = inr || d2[k] < mode.ext2;
                    if (cbase == 0) dmin[k] = fminf(dmin[k], d2[k]);
                }
#pragma unroll
                for (int k = 1; k < K; ++k)
                    if (d2[k] < d2[kmin]) kmin = k;
                const bool kept = real && (off ? inr : true);
                if (!kept) continue;
                if (cbase == 0 && pos[i] != 0) ++npos;
                const float xv = c < cin ? x[i * cin + c] : 0.0f;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    float wv = influence_of(d2[k], mode);
                    if (mode.closest && k != kmin) wv = 0.f;
                    acc[k] += wv * xv;
                }
            }
            if (c < cin)
#pragma unroll
                for (int k = 0; k < K; ++k) wf[(long)q * K * cin + (long)k * cin + c] = acc[k] * mod[k];
        }
        if (lane == 0) {
            inv_n[q] = 1.0f / (float)(npos > 1 ? npos : 1);
            if (min_d2)
#pragma unroll
                for (int k = 0; k < K; ++k) min_d2[(long)q * K + k] = dmin[k];
        }
    }
}


// ---- backward (pcrcg_kpconv_backward_ex, include/pcrcg_train.h) --------------------------------------------------------
// Given d_wf = dL/d wf of the (modulated) wf the forward stored, with diff = nb - kp_q, m = 2 sigmoid(off[q, 3K + k]) (1 when
// not modulated) and g[q,h,k] = sum_c d_wf[q,k,c] x[idx[q,h],c] over kept neighbours:
//   dx[idx[q,h], c]  += sum_k w m d_wf[q,k,c]
//   d_off[q, 3k + a]  = extent m sum_h g dw/dkp_a,    dw/dkp_a = linear   diff_a / (sqrt(d2) extent) where w > 0 and d2 > 0
//                                                                gaussian 2 w diff_a / (2 (0.3 extent)^2 + 1e-9);  constant 0
//   d_off[q, 3K + k]  = (sum_h w g) m (1 - m / 2)                (w before modulation: no division by an m that underflowed)
// The kept bit and the closest one-hot are constants, as in torch; n_q and min_d2 carry no gradient.  At d2 == 0 in linear
// mode torch gives NaN (0 * inf through sqrt's derivative); the zero subgradient is returned here.
//
// k_kpconv_ex_bwd_mfma: ONE WORKGROUP PER QUERY, one to four wavefronts, each taking 16-neighbour tiles in turn; d_wf[q]
// (15 x up to 512 channels, rows padded by 4 floats: the scalar operand read of the second product is conflict-free, the
// float4 read of the first has one two-way overlap per 16-lane phase) sits in LDS.  All
// per-(neighbour, kernel point) values live in one layout: lane (hsub, j) register r = neighbour j of the tile, kernel
// point 4 hsub + r (15: padding) -- d2, kept and the argmin are the forward's expressions on it.  Two products on
// v_mfma_f32_16x16x4_f32 share that tile:
//   g^T [16 kp x 16 nb] = d_wf [16 x cin] x^T [cin x 16]: A = LDS float4 of kernel point j, B = float4 of neighbour j's row
//        (channels 16 s + 4 hsub ..+3: each row is read once, 64 contiguous bytes per neighbour and step); D lands in the
//        layout above;
//   G [16 nb x 16 ch] = (w m) [16 x 16 kp] d_wf [16 kp x 16 ch] per 16-channel group: A = the tile's w m (K slot hsub of step
//        st = kernel point 4 hsub + st), B = LDS; D register r = neighbour 4 hsub + r: one scatter_add per (neighbour, channel).
// d_off is summed in a fixed order -- tiles in a lane, the 16 lanes of a kernel point by butterfly, the wavefronts through
// LDS by one thread per kernel point -- and stored: no atomics, the same bits every run.
constexpr int kBwdChunk = 512;     // channels of d_wf[q] in LDS at a time (wider inputs: the tile loop reloads per chunk)
constexpr int kBwdPad = 4;

template <bool DET>
__global__ void __launch_bounds__(256) k_kpconv_ex_bwd_mfma(
    const float* __restrict__ q_pts, int nq, const float* __restrict__ s_pts, int ns, const long long* __restrict__ idx, int H,
    int ld_idx, const float* __restrict__ x, int cin, const float* __restrict__ kp, const float* __restrict__ off, int ld_off,
    ExMode mode, const float* __restrict__ d_wf, float* __restrict__ dx, float* __restrict__ d_off, int ld_doff, int cchunk,
    FixAcc fx) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int stride = cchunk + kBwdPad;
    float* dws = lds;                           // [16][stride], row 15 zero
    float* red = lds + 16 * stride;             // [waves][16 kernel points][4]
    const int lane = threadIdx.x & 63;
    const int hsub = lane >> 4, j = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nw = (int)(blockDim.x >> 6);
    const int q = blockIdx.x;
    const double fscale = DET ? fix_scale(fx) : 1.0;
    const bool deform = off != nullptr;
    const bool want_g = d_off != nullptr, want_dx = dx != nullptr;
    const float qx = q_pts[3 * (long)q], qy = q_pts[3 * (long)q + 1], qz = q_pts[3 * (long)q + 2];
    float kpx[4], kpy[4], kpz[4], mod[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int k = 4 * hsub + r, kc = k < K ? k : K - 1;
        kpx[r] = kp[3 * kc]; kpy[r] = kp[3 * kc + 1]; kpz[r] = kp[3 * kc + 2];
        if (deform) {
            const float* o = off + (long)q * ld_off + 3 * kc;
            kpx[r] = deformed(o[0], mode.extent, kpx[r]);
            kpy[r] = deformed(o[1], mode.extent, kpy[r]);
            kpz[r] = deformed(o[2], mode.extent, kpz[r]);
        }
        mod[r] = mode.modulated ? modulation(off, q, ld_off, kc) : 1.0f;
    }
    for (int c = threadIdx.x; c < stride; c += blockDim.x) dws[15 * stride + c] = 0.f;
    float sx[4] = {0.f, 0.f, 0.f, 0.f}, sy[4] = {0.f, 0.f, 0.f, 0.f}, sz[4] = {0.f, 0.f, 0.f, 0.f}, sm[4] = {0.f, 0.f, 0.f, 0.f};
    const int ntiles = (H + 15) / 16, nrounds = (ntiles + nw - 1) / nw, nchunks = (cin + cchunk - 1) / cchunk;
    const float* dq = d_wf + (long)q * K * cin;

    for (int round = 0; round < nrounds; ++round) {
        const int tile = round * nw + wave;
        const int h = tile * 16 + j;
        const long long iv = idx[(long)q * ld_idx + (h < H ? h : H - 1)];
        const int i = (h < H && iv >= 0 && iv < ns) ? (int)iv : -1;
        const long ic = i >= 0 ? i : 0;
        const float px = s_pts[3 * ic] - qx, py = s_pts[3 * ic + 1] - qy, pz = s_pts[3 * ic + 2] - qz;
        float d2[4], ddx[4], ddy[4], ddz[4];
        bool inr = false;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            ddx[r] = px - kpx[r]; ddy[r] = py - kpy[r]; ddz[r] = pz - kpz[r];
            d2[r] = (i >= 0 && 4 * hsub + r < K) ? ddx[r] * ddx[r] + ddy[r] * ddy[r] + ddz[r] * ddz[r] : INFINITY;
            inr = inr || d2[r] < mode.ext2;
        }
        bool kept = i >= 0;
        if (deform) {
            const unsigned long long b = __ballot(inr);
            kept = ((b >> j) & 0x0001000100010001ull) != 0ull;
        }
        int bk = 4 * hsub;
        if (mode.closest) {
            float bd = d2[0];
#pragma unroll
            for (int r = 1; r < 4; ++r)
                if (d2[r] < bd) { bd = d2[r]; bk = 4 * hsub + r; }
#pragma unroll
            for (int m = 16; m < 64; m <<= 1) {
                const float od = __shfl_xor(bd, m, 64);
                const int ok = __shfl_xor(bk, m, 64);
                const bool take = argmin_takes(od, ok, bd, bk);
                bd = take ? od : bd;
                bk = take ? ok : bk;
            }
        }
        float w[4], am[4], dwx[4], dwy[4], dwz[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = 4 * hsub + r;
            float wv = influence_of(d2[r] == INFINITY ? 0.f : d2[r], mode);
            if (mode.closest && bk != k) wv = 0.f;
            w[r] = (kept && k < K) ? wv : 0.f;
            am[r] = w[r] * mod[r];
            float f = 0.f;                                   // dw/dkp_a = f * diff_a
            if (mode.influence == 1) f = (w[r] > 0.f && d2[r] > 0.f) ? 1.0f / (sqrtf(d2[r]) * mode.extent) : 0.f;
            else if (mode.influence == 2) f = 2.0f * w[r] / mode.gauss_den;
            dwx[r] = w[r] != 0.f ? f * ddx[r] : 0.f;
            dwy[r] = w[r] != 0.f ? f * ddy[r] : 0.f;
            dwz[r] = w[r] != 0.f ? f * ddz[r] : 0.f;
        }
        const int ik = kept ? i : -1;
        int ir[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) ir[r] = __shfl(ik, 4 * hsub + r, 64);
        const bool any_kept = __ballot(kept) != 0ull;
        f32x4 gacc = {0.f, 0.f, 0.f, 0.f};

        for (int chunk = 0; chunk < nchunks; ++chunk) {
            const int cc0 = chunk * cchunk;
            const int cw = cin - cc0 < cchunk ? cin - cc0 : cchunk;
            if (nchunks > 1 || round == 0) {
                __syncthreads();
                const int per_row = cw >> 2;
                for (int t = threadIdx.x; t < K * per_row; t += blockDim.x) {
                    const int k = t / per_row, c4 = t - k * per_row;
                    *reinterpret_cast<float4*>(dws + k * stride + 4 * c4) = *reinterpret_cast<const float4*>(dq + (long)k * cin + cc0 + 4 * c4);
                }
                __syncthreads();
            }
            if (!any_kept) continue;
            if (want_g) {
                const float* xrow = x + (long)(kept ? i : 0) * cin + cc0;
                for (int c16 = 0; c16 < cw; c16 += 16) {           // (wave-uniform trip count: a tail group is zero-filled)
                    const int c = c16 + 4 * hsub;
                    const bool ok = c < cw;
                    float4 a = *reinterpret_cast<const float4*>(dws + j * stride + (ok ? c : 0));
                    float4 b = *reinterpret_cast<const float4*>(xrow + (ok ? c : 0));
                    if (!ok) a = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (!ok || !kept) b = make_float4(0.f, 0.f, 0.f, 0.f);
                    gacc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, gacc, 0, 0, 0);
                    gacc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, gacc, 0, 0, 0);
                    gacc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, gacc, 0, 0, 0);
                    gacc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, gacc, 0, 0, 0);
                }
            }
            if (want_dx) {
                for (int c16 = 0; c16 < cw; c16 += 16) {
                    const int c = c16 + j;
                    const bool cok = c < cw;
                    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int st = 0; st < 4; ++st) {
                        const float b = cok ? dws[(4 * hsub + st) * stride + c] : 0.f;
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(am[st], b, acc, 0, 0, 0);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (ir[r] >= 0 && cok) scatter_add<DET>(dx, (long)ir[r] * cin + cc0 + c, acc[r], fx, fscale);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            sx[r] += gacc[r] * dwx[r];
            sy[r] += gacc[r] * dwy[r];
            sz[r] += gacc[r] * dwz[r];
            sm[r] += gacc[r] * w[r];
        }
    }
    if (!want_g) return;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) {
            sx[r] += __shfl_xor(sx[r], m, 64);
            sy[r] += __shfl_xor(sy[r], m, 64);
            sz[r] += __shfl_xor(sz[r], m, 64);
            sm[r] += __shfl_xor(sm[r], m, 64);
        }
    if (j == 0)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            *reinterpret_cast<float4*>(red + ((wave * 16) + 4 * hsub + r) * 4) = make_float4(sx[r], sy[r], sz[r], sm[r]);
    __syncthreads();
    if (threadIdx.x < K) {
        const int k = threadIdx.x;
        float4 s = *reinterpret_cast<const float4*>(red + k * 4);
        for (int wv = 1; wv < nw; ++wv) {
            const float4 t = *reinterpret_cast<const float4*>(red + (wv * 16 + k) * 4);
            s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
        }
        const float m = mode.modulated ? modulation(off, q, ld_off, k) : 1.0f;
        float* o = d_off + (long)q * ld_doff;
        const float em = mode.extent * m;
        o[3 * k] = em * s.x;
        o[3 * k + 1] = em * s.y;
        o[3 * k + 2] = em * s.z;
        if (mode.modulated) o[3 * K + k] = s.w * (m * (1.0f - 0.5f * m));
    }
}

// Plain restatement for cin == 1, channel counts that are no multiple of 4 and unaligned rows: one wavefront per query,
// lanes = neighbours, kernel points in turn; correct, not fast (every lane re-derives its neighbour's kept bit and argmin
// for every kernel point, and the scatter takes one add per (neighbour, kernel point, channel)).
template <bool DET>
__global__ void __launch_bounds__(kWavesPerBlock * 64) k_kpconv_ex_bwd_scalar(
    const float* __restrict__ q_pts, int nq, const float* __restrict__ s_pts, int ns, const long long* __restrict__ idx, int H,
    int ld_idx, const float* __restrict__ x, int cin, const float* __restrict__ kp, const float* __restrict__ off, int ld_off,
    ExMode mode, const float* __restrict__ d_wf, float* __restrict__ dx, float* __restrict__ d_off, int ld_doff, FixAcc fx) {
    const int lane = threadIdx.x & 63;
    const long q = (long)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (q >= nq) return;
    const double fscale = DET ? fix_scale(fx) : 1.0;
    const float qx = q_pts[3 * q], qy = q_pts[3 * q + 1], qz = q_pts[3 * q + 2];
    for (int k = 0; k < K; ++k) {
        const float m = mode.modulated ? modulation(off, q, ld_off, k) : 1.0f;
        const float* dk = d_wf + (q * K + k) * cin;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        for (int hc = 0; hc < H; hc += 64) {
            const int h = hc + lane;
            const long long iv = h < H ? idx[q * ld_idx + h] : -1;
            const bool real = iv >= 0 && iv < ns;
            const long i = real ? (long)iv : 0;
            const float nx = (real ? s_pts[3 * i] : kShadow) - qx, ny = (real ? s_pts[3 * i + 1] : kShadow) - qy,
                        nz = (real ? s_pts[3 * i + 2] : kShadow) - qz;
            bool inr = false;
            int kmin = 0;
            float best = INFINITY, d2k = 0.f, ex = 0.f, ey = 0.f, ez = 0.f;
            for (int kk = 0; kk < K; ++kk) {
                float kx = kp[3 * kk], ky = kp[3 * kk + 1], kz = kp[3 * kk + 2];
                if (off) {
                    const float* o = off + q * ld_off + 3 * kk;
                    kx = deformed(o[0], mode.extent, kx);
                    ky = deformed(o[1], mode.extent, ky);
                    kz = deformed(o[2], mode.extent, kz);
                }
                const float ddx = nx - kx, ddy = ny - ky, ddz = nz - kz;
                const float d = ddx * ddx + ddy * ddy + ddz * ddz;
                inr = inr || d < mode.ext2;
                if (d < best) { best = d; kmin = kk; }
                if (kk == k) { d2k = d; ex = ddx; ey = ddy; ez = ddz; }
            }
            const bool kept = real && (off ? inr : true);
            float wv = kept ? influence_of(d2k, mode) : 0.f;
            if (mode.closest && kmin != k) wv = 0.f;
            if (wv != 0.f) {
                float g = 0.f;
                for (int c = 0; c < cin; ++c) {
                    const float dv = dk[c];
                    g += dv * x[i * cin + c];
                    if (dx) scatter_add<DET>(dx, i * cin + c, wv * m * dv, fx, fscale);
                }
                float f = 0.f;
                if (mode.influence == 1) f = d2k > 0.f ? 1.0f / (sqrtf(d2k) * mode.extent) : 0.f;
                else if (mode.influence == 2) f = 2.0f * wv / mode.gauss_den;
                s0 += g * (f * ex);
                s1 += g * (f * ey);
                s2 += g * (f * ez);
                s3 += g * wv;
            }
        }
        if (!d_off) continue;
#pragma unroll
        for (int mk = 1; mk < 64; mk <<= 1) {
            s0 += __shfl_xor(s0, mk, 64);
            s1 += __shfl_xor(s1, mk, 64);
            s2 += __shfl_xor(s2, mk, 64);
            s3 += __shfl_xor(s3, mk, 64);
        }
        if (lane == 0) {
            float* o = d_off + q * ld_doff;
            const float em = mode.extent * m;
            o[3 * k] = em * s0;
            o[3 * k + 1] = em * s1;
            o[3 * k + 2] = em * s2;
            if (mode.modulated) o[3 * K + k] = s3 * (m * (1.0f - 0.5f * m));
        }
    }
}

}  // namespace
}  // namespace pcrcg

using namespace pcrcg;

// the mode constants of one call, the same for the forward and the backward entry
static ExMode ex_mode(float extent, int influence, int closest, int modulated) {
    ExMode mode;
    mode.influence = influence;
    mode.closest = closest;
    mode.modulated = modulated;
    mode.extent = extent;
    mode.ext2 = extent * extent;
    const double sigma = 0.3 * (double)extent;
    mode.gauss_den = (float)(2.0 * sigma * sigma + 1e-9);
    return mode;
}

// the argument checks of both entries; the pointers are looked at before the empty-call exit (each entry adds its own)
static int ex_check(const float* q_pts, int nq, const float* s_pts, int ns, const int64_t* idx, int h, int ld_idx, const float* x,
                    int cin, const float* kp, float extent, const float* offset_features, int ld_off, int influence, int closest,
                    int modulated) {
    PCRCG_CHECK_ARG(nq >= 0 && ns >= 1 && h >= 1 && ld_idx >= h && cin >= 1);
    PCRCG_CHECK_ARG(extent > 0.0f);
    PCRCG_CHECK_ARG(influence >= 0 && influence <= 2);
    PCRCG_CHECK_ARG((closest == 0 || closest == 1) && (modulated == 0 || modulated == 1));
    PCRCG_CHECK_ARG(q_pts && s_pts && idx && x && kp);
    PCRCG_CHECK_ARG(offset_features || !modulated);
    PCRCG_CHECK_ARG(!offset_features || ld_off >= (modulated ? 4 : 3) * K);
    return PCRCG_OK;
}

extern "C" int pcrcg_kpconv_aggregate_ex(const float* q_pts, int nq, const float* s_pts, int ns, const int64_t* idx, int h,
                                         int ld_idx, const float* x, int cin, const float* kp, float extent,
                                         const float* offset_features, int ld_off, int influence, int closest, int modulated,
                                         float* wf, float* inv_n, float* min_d2, void* ws, size_t ws_bytes, void* stream) {
    PCRCG_PROPAGATE(ex_check(q_pts, nq, s_pts, ns, idx, h, ld_idx, x, cin, kp, extent, offset_features, ld_off, influence, closest,
                             modulated));
    PCRCG_CHECK_ARG(wf && inv_n && ws);
    if (nq == 0) return PCRCG_OK;
    hipStream_t st = as_stream(stream);
    KpWs w;
    PCRCG_PROPAGATE(kpconv_ws(ws, ws_bytes, ns, &w));
    PCRCG_PROPAGATE(kpconv_pack(x, ns, cin, s_pts, w, st));
    const ExMode mode = ex_mode(extent, influence, closest, modulated);
    const long long* idx_ll = reinterpret_cast<const long long*>(idx);
    if (!kpconv_vec_ok(cin, x, wf)) {
        hipLaunchKernelGGL(k_kpconv_ex_scalar, dim3(kpconv_blocks(nq)), dim3(kWavesPerBlock * 64), 0, st, q_pts, nq, s_pts, ns,
                           idx_ll, h, ld_idx, x, cin, kp, offset_features, ld_off, mode, (const unsigned char*)w.pos, wf, inv_n,
                           min_d2);
        PCRCG_CHECK_LAUNCH();
        return PCRCG_OK;
    }
    const KpPlan p = kpconv_plan(nq, cin, false, false);
#define LAUNCH(NBV)                                                                                                         \
    hipLaunchKernelGGL((k_kpconv_ex_mfma<NBV>), dim3(p.blocks), dim3(kWavesPerBlock * 64), 0, st, q_pts, nq, ns, idx_ll, h,  \
                       ld_idx, x, cin, kp, offset_features, ld_off, mode, (const float4*)w.pk, wf, inv_n, min_d2, p.nchunk)
    if (p.nb == 4) LAUNCH(4);
    else if (p.nb == 2) LAUNCH(2);
    else LAUNCH(1);
#undef LAUNCH
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}

extern "C" int pcrcg_kpconv_backward_ex(const float* q_pts, int nq, const float* s_pts, int ns, const int64_t* idx, int h,
                                        int ld_idx, const float* x, int cin, const float* kp, float extent,
                                        const float* offset_features, int ld_off, int influence, int closest, int modulated,
                                        const float* d_wf, float* dx, float* d_off, int ld_doff, void* stream) {
    PCRCG_PROPAGATE(ex_check(q_pts, nq, s_pts, ns, idx, h, ld_idx, x, cin, kp, extent, offset_features, ld_off, influence, closest,
                             modulated));
    PCRCG_CHECK_ARG(d_wf);
    PCRCG_CHECK_ARG(!d_off || (offset_features && ld_doff >= (modulated ? 4 : 3) * K));
    if (nq == 0 || (!dx && !d_off)) return PCRCG_OK;
    hipStream_t st = as_stream(stream);
    const ExMode mode = ex_mode(extent, influence, closest, modulated);
    const long long* ix = reinterpret_cast<const long long*>(idx);
    const bool aligned = kpconv_vec_ok(cin, x, d_wf);
    const int cchunk = cin < kBwdChunk ? (cin + 3) / 4 * 4 : kBwdChunk;
    const int nwaves = (h + 15) / 16 < 4 ? (h + 15) / 16 : 4;
    const size_t lds_bytes = ((size_t)16 * (cchunk + kBwdPad) + 4 * 16 * 4) * sizeof(float);
    auto run = [&](auto det, const FixAcc& fx) {
        constexpr bool DET = decltype(det)::value;
        if (aligned)
            hipLaunchKernelGGL(k_kpconv_ex_bwd_mfma<DET>, dim3((unsigned)nq), dim3(64 * nwaves), lds_bytes, st, q_pts, nq, s_pts, ns,
                               ix, h, ld_idx, x, cin, kp, offset_features, ld_off, mode, d_wf, dx, d_off, ld_doff, cchunk, fx);
        else
            hipLaunchKernelGGL(k_kpconv_ex_bwd_scalar<DET>, dim3((unsigned)((nq + kWavesPerBlock - 1) / kWavesPerBlock)),
                               dim3(kWavesPerBlock * 64), 0, st, q_pts, nq, s_pts, ns, ix, h, ld_idx, x, cin, kp, offset_features,
                               ld_off, mode, d_wf, dx, d_off, ld_doff, fx);
    };
    if (dx) {
        // |contribution| <= 15 * 2 max|d_wf| (influence weights <= 1, modulation <= 2), at most nq of them per element
        return scatter_launch(st, (size_t)ns * cin, {d_wf, nq, K * cin, (long)K * cin}, 23, {}, dx, run);
    }
    run(std::false_type(), FixAcc{nullptr, nullptr, 0, nullptr});
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}
