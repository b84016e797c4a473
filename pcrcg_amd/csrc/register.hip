// register.hip -- the registration back end on gfx950: feature matching and RANSAC over the correspondences.
// ABI: include/pcrcg.h, section "Registration back end".
//
// Replaces ransac_pose_estimation (ref:lib/benchmark_utils.py:187-224), i.e. open3d 0.10's
// registration_ransac_based_on_feature_matching / _based_on_correspondence, with a deterministic algorithm of the same
// structure (DESIGN.md section 10 states it in full; tests/ransac_ref.py restates it in numpy):
//
//   match     : non-mutual -- every source point i is paired with its nearest target in L2 feature distance, the
//               arg-max over j of <a_i, b_j> - |b_j|^2 / 2 (fp32; lowest j on ties); mutual -- the pairs that are the
//               arg-max of <a_i, b_j> along both their row and their column (pcrcg_feature_argmax both ways + one
//               compaction), in ascending source order.  The count K stays on the device.
//   hypotheses: one thread per hypothesis h, float64 -- ransac_n rows drawn from the list by splitmix64, distinct source
//               ids, edge-length check, Kabsch fit with the reflection fix (one-sided Jacobi SVD of the 3 x 3
//               cross-covariance), degeneracy test, distance check; a pass flag and the fp32-rounded R|t.
//   compaction: the first max_validation passing hypotheses in index order (device-wide scan of the flags).
//   evaluation: one workgroup per validated hypothesis; every source point is moved with unfused fp32 arithmetic and
//               looked up in the target's cell grid (27 cells around it); count and float64 sum of the nearest d2 over the
//               inliers (d2 < thr2), reduced in a fixed order -- bit-reproducible.
//   selection : highest count, then lowest sum, then lowest h; the float64 transform of the winner is re-fitted from its
//               samples (the same device function) and written with the statistics.
//
// Several pairs per call (pcrcg_feature_match_batch, pcrcg_ransac_batch): the same stages with the pair as a grid
// dimension, each kernel running the single-pair device code (the inline bodies below and hypothesis()) on a per-pair
// view, one device-wide scan over all pairs' flags; so pair b's result is the single-pair result bit for bit.
//
// Compiled with -ffp-contract=off: every fp32 and fp64 operation rounds where the source says, so the numpy restatement
// reproduces the evaluation's counts exactly.
#include "argmax.h"
#include "block_scan.h"
#include "cellgrid.h"
#include "common.h"
#include "kabsch.h"
#include "pcrcg_train.h"
#include "splitmix.h"

namespace pcrcg {
namespace {

constexpr int kMaxSample = 8;         // ransac_n <= 8: the draws of hypothesis h are 8 h .. 8 h + 7
constexpr int kEvalThreads = 512;     // evaluation workgroup: one validated hypothesis

// (score, column) as one orderable word: a larger score wins, an equal score keeps the smaller column
__device__ inline u64 pack_max(float v, int j) {
    const unsigned b = __float_as_uint(v);
    const unsigned key = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((u64)key << 32) | (u64)(0xFFFFFFFFu - (unsigned)j);
}

// ---- L2 nearest neighbour in feature space -------------------------------------------------------------------------
// argmin_j |a - b_j|^2 = argmax_j <a, b_j> - |b_j|^2 / 2.  hb[j] = |b_j|^2 / 2, summed in order.
__global__ void __launch_bounds__(256) k_half_norms(const float* __restrict__ b, int ldb, int m, int c, float* __restrict__ hb) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    float s = 0.f;
    for (int k = 0; k < c; ++k) {
        const float v = b[(long)j * ldb + k];
        s = s + v * v;
    }
    hb[j] = 0.5f * s;
}

// C = 32 or 64 on the fp32 matrix cores, laid out like k_feature_argmax_mfma32 (trainops.hip): a wavefront holds 32 rows of
// A as its operand (lane (row, half) keeps A[row][C/2 half + s]) and walks its column range 32 columns at a time, C/2
// v_mfma_f32_32x32x2_f32 per 32 x 32 block of dot products; each lane keeps the best (dot - hb) of its 16 rows over the
// columns congruent to its lane index (strictly greater: the smaller column survives a tie), the 32 lanes of a row meet by
// shuffles, and the column ranges (grid.y) by a 64-bit atomicMax.
typedef float rg_f16 __attribute__((ext_vector_type(16)));
// The body is shared with the batch kernel (pair = grid.z): bx / by are the row block and the column range.
template <int C>
__device__ __forceinline__ void l2nn_mfma_tile(const float* a, int lda, int n, const float* b, int ldb,
                                               int m, const float* hb, int cols_per, u64* packed,
                                               unsigned bx, unsigned by) {
    constexpr int NV = C / 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const int row0 = (bx * 4 + wave) * 32;
    if (row0 >= n) return;
    const int jbeg = by * cols_per, jend = min(m, jbeg + cols_per);
    if (jbeg >= jend) return;
    float av[NV];
    {
        const float* ap = a + (long)min(row0 + l31, n - 1) * lda + NV * half;
#pragma unroll
        for (int q = 0; q < NV / 4; ++q) {
            const float4 t = *reinterpret_cast<const float4*>(ap + 4 * q);
            av[4 * q] = t.x; av[4 * q + 1] = t.y; av[4 * q + 2] = t.z; av[4 * q + 3] = t.w;
        }
    }
    float best[16];
    int bj[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { best[r] = -INFINITY; bj[r] = 0; }
    for (int j0 = jbeg; j0 < jend; j0 += 32) {
        const int col = j0 + l31;
        const int cc = min(col, m - 1);
        float bv[NV];
        const float* bp = b + (long)cc * ldb + NV * half;
#pragma unroll
        for (int q = 0; q < NV / 4; ++q) {
            const float4 t = *reinterpret_cast<const float4*>(bp + 4 * q);
            bv[4 * q] = t.x; bv[4 * q + 1] = t.y; bv[4 * q + 2] = t.z; bv[4 * q + 3] = t.w;
        }
        const float h = hb[cc];
        rg_f16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int s2 = 0; s2 < NV; ++s2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s2], bv[s2], acc, 0, 0, 0);
        if (col < jend) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float s = acc[r] - h;
                if (s > best[r]) { best[r] = s; bj[r] = col; }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        u64 p = pack_max(best[r], bj[r]);
#pragma unroll
        for (int sh = 16; sh >= 1; sh >>= 1) {
            const u64 o = __shfl_xor(p, sh, 64);
            p = o > p ? o : p;
        }
        const int row = row0 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (l31 == 0 && row < n) atomicMax(&packed[row], p);
    }
}

template <int C>
__global__ void __launch_bounds__(256) k_l2nn_mfma(const float* __restrict__ a, int lda, int n, const float* __restrict__ b,
                                                   int ldb, int m, const float* __restrict__ hb, int cols_per,
                                                   u64* __restrict__ packed) {
    l2nn_mfma_tile<C>(a, lda, n, b, ldb, m, hb, cols_per, packed, blockIdx.x, blockIdx.y);
}

// several pairs: pair p = blockIdx.z owns source rows a_off[p] .. a_off[p+1] and target rows b_off[p] .. b_off[p+1]; its
// column indices are local to the pair
template <int C>
__global__ void __launch_bounds__(256) k_l2nn_mfma_batch(const float* __restrict__ a, int lda, const int* __restrict__ a_off,
                                                         const float* __restrict__ b, int ldb, const int* __restrict__ b_off,
                                                         const float* __restrict__ hb, int cols_per, u64* __restrict__ packed) {
    const int p = blockIdx.z;
    const int i0 = a_off[p], j0 = b_off[p];
    l2nn_mfma_tile<C>(a + (long)i0 * lda, lda, a_off[p + 1] - i0, b + (long)j0 * ldb, ldb, b_off[p + 1] - j0, hb + j0, cols_per,
                      packed + i0, blockIdx.x, blockIdx.y);
}

// any width (and unaligned operands): one thread per row of A, a column range per grid.y
__device__ __forceinline__ void l2nn_any_row(const float* a, int lda, int n, const float* b, int ldb,
                                             int m, int c, const float* hb, int cols_per, u64* packed,
                                             int row, unsigned by) {
    if (row >= n) return;
    const int jbeg = by * cols_per, jend = min(m, jbeg + cols_per);
    if (jbeg >= jend) return;
    float bv = -INFINITY;
    int bj = jbeg;
    for (int j = jbeg; j < jend; ++j) {
        float s = 0.f;
        for (int k = 0; k < c; ++k) s = fmaf(a[(long)row * lda + k], b[(long)j * ldb + k], s);
        s = s - hb[j];
        if (s > bv) { bv = s; bj = j; }
    }
    atomicMax(&packed[row], pack_max(bv, bj));
}

__global__ void __launch_bounds__(256) k_l2nn_any(const float* __restrict__ a, int lda, int n, const float* __restrict__ b,
                                                  int ldb, int m, int c, const float* __restrict__ hb, int cols_per,
                                                  u64* __restrict__ packed) {
    l2nn_any_row(a, lda, n, b, ldb, m, c, hb, cols_per, packed, blockIdx.x * 256 + threadIdx.x, blockIdx.y);
}

__global__ void __launch_bounds__(256) k_l2nn_any_batch(const float* __restrict__ a, int lda, const int* __restrict__ a_off,
                                                        const float* __restrict__ b, int ldb, const int* __restrict__ b_off, int c,
                                                        const float* __restrict__ hb, int cols_per, u64* __restrict__ packed) {
    const int p = blockIdx.z;
    const int i0 = a_off[p], j0 = b_off[p];
    l2nn_any_row(a + (long)i0 * lda, lda, a_off[p + 1] - i0, b + (long)j0 * ldb, ldb, b_off[p + 1] - j0, c, hb + j0, cols_per,
                 packed + i0, blockIdx.x * 256 + threadIdx.x, blockIdx.y);
}

// non-mutual list: row i = (i, nn(i)), K = n
__global__ void __launch_bounds__(256) k_nn_emit(const u64* __restrict__ packed, int n, int* __restrict__ corr, int* __restrict__ k) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) *k = n;
    if (i >= n) return;
    corr[2 * i] = i;
    corr[2 * i + 1] = (int)(0xFFFFFFFFu - (unsigned)(packed[i] & 0xFFFFFFFFull));
}

// the same per pair (grid.y): rows of pair p at off[p] .., indices local to the pair, k[p] = its length
__global__ void __launch_bounds__(256) k_nn_emit_batch(const u64* __restrict__ packed, const int* __restrict__ off,
                                                       int* __restrict__ corr, int* __restrict__ k) {
    const int p = blockIdx.y, i0 = off[p], n = off[p + 1] - i0;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) k[p] = n;
    if (i >= n) return;
    corr[2 * (long)(i0 + i)] = i;
    corr[2 * (long)(i0 + i) + 1] = (int)(0xFFFFFFFFu - (unsigned)(packed[i0 + i] & 0xFFFFFFFFull));
}

// mutual list: i is kept iff the arg-max of its row points at a column whose arg-max is i
__global__ void __launch_bounds__(256) k_mutual_flags(const long long* __restrict__ arg_s, int n, const long long* __restrict__ arg_t,
                                                      int* __restrict__ flags) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    flags[i] = arg_t[arg_s[i]] == i ? 1 : 0;
}

__global__ void __launch_bounds__(256) k_mutual_emit(const int* __restrict__ flags, const int* __restrict__ offs, int n,
                                                     const long long* __restrict__ arg_s, int* __restrict__ corr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !flags[i]) return;
    const int o = offs[i];
    corr[2 * o] = i;
    corr[2 * o + 1] = (int)arg_s[i];
}

// the mutual L2 list of ragged pairs (pcrcg_mutual_match_batch): one workgroup per pair walks its source rows 256 at a time,
// ps / pt the packed arg-max words of the rows (source -> target) and of the columns (target -> source).  Row i is kept iff
// its column's arg-max is i; a block scan ranks a round's kept rows, so the list is in ascending i.  Rows k .. n - 1 of the
// pair get (-1, -1).  (A kept row is written at or before its own place, the tail after the walk: corr is never read.)
__global__ void __launch_bounds__(256) k_mutual_emit_batch(const u64* __restrict__ ps, const int* __restrict__ s_off,
                                                           const u64* __restrict__ pt, const int* __restrict__ t_off,
                                                           int* __restrict__ corr, int* __restrict__ k) {
    __shared__ int s_scan[4];
    const int p = blockIdx.x;
    const int i0 = s_off[p], n = s_off[p + 1] - i0;
    const int j0 = t_off[p], m = t_off[p + 1] - j0;
    int kept = 0;
    if (m > 0) {
        for (int base = 0; base < n; base += 256) {
            const int i = base + (int)threadIdx.x;
            int j = -1;
            bool keep = false;
            if (i < n) {
                j = (int)(0xFFFFFFFFu - (unsigned)(ps[i0 + i] & 0xFFFFFFFFull));
                keep = j >= 0 && j < m && (int)(0xFFFFFFFFu - (unsigned)(pt[j0 + j] & 0xFFFFFFFFull)) == i;
            }
            int total;
            const int rank = block_excl_scan_i32<256>(keep ? 1 : 0, &total, s_scan);
            if (keep) {
                corr[2 * (long)(i0 + kept + rank)] = i;
                corr[2 * (long)(i0 + kept + rank) + 1] = j;
            }
            kept += total;
        }
    }
    for (int i = kept + (int)threadIdx.x; i < n; i += 256) {
        corr[2 * (long)(i0 + i)] = -1;
        corr[2 * (long)(i0 + i) + 1] = -1;
    }
    if (threadIdx.x == 0) k[p] = kept;
}

// ---- hypotheses ----------------------------------------------------------------------------------------------------
struct HypArgs {
    const float* src;
    const float* tgt;
    const int* corr;
    const int* k;
    int k_max, ransac_n, dist_check, max_iteration;
    double thr, sim;
    u64 seed;
};

__device__ inline int list_size(const HypArgs& a) {
    const int k = *a.k;
    return k < 0 ? 0 : (k > a.k_max ? a.k_max : k);
}

__device__ inline void load3(const float* p, int i, double* v) {
    v[0] = p[3 * (long)i]; v[1] = p[3 * (long)i + 1]; v[2] = p[3 * (long)i + 2];
}

__device__ inline double dist3(const double* p, const double* q) {
    const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

// Hypothesis h: the drawn rows (rows[]), then every check in the documented order; R (row-major) and t receive the fit
// (zero when the hypothesis fails before it).  Returns the pass flag.
__device__ bool hypothesis(const HypArgs& a, int h, int K, int* rows, double* R, double* t) {
    for (int e = 0; e < 9; ++e) R[e] = 0.0;
    t[0] = t[1] = t[2] = 0.0;
    const int ns = a.ransac_n;
    for (int s = 0; s < ns; ++s) {
        const u64 r = splitmix64((a.seed << 40) + 8ull * (u64)h + (u64)s);
        rows[s] = (int)(((r >> 32) * (u64)K) >> 32);
    }
    if (K < ns) return false;
    double ps[kMaxSample][3], pt[kMaxSample][3];
    int sid[kMaxSample];
    for (int s = 0; s < ns; ++s) {
        sid[s] = a.corr[2 * rows[s]];
        load3(a.src, sid[s], ps[s]);
        load3(a.tgt, a.corr[2 * rows[s] + 1], pt[s]);
    }
    for (int i = 0; i < ns; ++i)
        for (int j = i + 1; j < ns; ++j)
            if (sid[i] == sid[j]) return false;
    if (a.sim > 0.0) {
        for (int i = 0; i < ns; ++i)
            for (int j = i + 1; j < ns; ++j) {
                const double ds = dist3(ps[i], ps[j]), dt = dist3(pt[i], pt[j]);
                if (ds < dt * a.sim || dt < ds * a.sim) return false;
            }
    }
    // Kabsch: centroids, H = sum (ps - cs)(pt - ct)^T, H = U S V^T, R = V diag(1, 1, det(V U^T)) U^T, t = ct - R cs
    double cs[3] = {0.0, 0.0, 0.0}, ct[3] = {0.0, 0.0, 0.0};
    for (int s = 0; s < ns; ++s)
        for (int d = 0; d < 3; ++d) { cs[d] += ps[s][d]; ct[d] += pt[s][d]; }
    for (int d = 0; d < 3; ++d) { cs[d] /= ns; ct[d] /= ns; }
    double H[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    for (int s = 0; s < ns; ++s)
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) H[r][c] += (ps[s][r] - cs[r]) * (pt[s][c] - ct[c]);
    if (!kabsch_from_covariance(H, cs, ct, R, t)) return false;
    if (a.dist_check) {
        for (int s = 0; s < ns; ++s) {
            double q[3];
            for (int r = 0; r < 3; ++r) q[r] = ((R[3 * r] * ps[s][0] + R[3 * r + 1] * ps[s][1]) + R[3 * r + 2] * ps[s][2]) + t[r];
            if (!(dist3(q, pt[s]) <= a.thr)) return false;
        }
    }
    return true;
}

__global__ void __launch_bounds__(256) k_hypotheses(HypArgs a, int* __restrict__ pass, float* __restrict__ xf,
                                                    int* __restrict__ tr_samples, int* __restrict__ tr_pass,
                                                    float* __restrict__ tr_xf32, double* __restrict__ tr_xf64) {
    const int h = blockIdx.x * 256 + threadIdx.x;
    if (h >= a.max_iteration) return;
    int rows[kMaxSample];
    double R[9], t[3];
    const bool ok = hypothesis(a, h, list_size(a), rows, R, t);
    pass[h] = ok ? 1 : 0;
    float f[12];
    for (int e = 0; e < 9; ++e) f[e] = (float)R[e];
    for (int e = 0; e < 3; ++e) f[9 + e] = (float)t[e];
    for (int e = 0; e < 12; ++e) xf[12 * (long)h + e] = f[e];
    if (tr_samples)
        for (int s = 0; s < a.ransac_n; ++s) tr_samples[(long)h * a.ransac_n + s] = rows[s];
    if (tr_pass) tr_pass[h] = ok ? 1 : 0;
    if (tr_xf32)
        for (int e = 0; e < 12; ++e) tr_xf32[12 * (long)h + e] = f[e];
    if (tr_xf64) {
        for (int e = 0; e < 9; ++e) tr_xf64[12 * (long)h + e] = R[e];
        for (int e = 0; e < 3; ++e) tr_xf64[12 * (long)h + 9 + e] = t[e];
    }
}

// the first max_validation passing hypotheses (offs = exclusive scan of the flags)
__global__ void __launch_bounds__(256) k_compact(const int* __restrict__ pass, const int* __restrict__ offs, int max_iteration,
                                                 int max_validation, int* __restrict__ vid, int* __restrict__ tr_vid) {
    const int h = blockIdx.x * 256 + threadIdx.x;
    if (h >= max_iteration || !pass[h]) return;
    const int o = offs[h];
    if (o < max_validation) {
        vid[o] = h;
        if (tr_vid) tr_vid[o] = h;
    }
}

// ---- evaluation: one workgroup per validated hypothesis ----------------------------------------------------------
// The workgroup's count and float64 sum of the inliers of transform xf[0..11] over src [n, 3]; the target cloud is m
// supports whose hash table is the 2 m slots at tab.  Shared by k_evaluate and k_evaluate_batch; the totals are left in
// s_c[0] / s_s[0].
__device__ __forceinline__ void evaluate_block(const float* src, int n, const GridView& g, const Slot* tab, int m,
                                               float thr2, const float* xf, int* s_c, double* s_s) {
    float T[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) T[e] = xf[e];
    const double inv_cell = g.hdr->inv_cell;
    const unsigned tsize = 2u * (unsigned)m;
    int cnt = 0;
    double sum = 0.0;
    for (int i = threadIdx.x; i < n && m > 0; i += kEvalThreads) {
        const float x = src[3 * (long)i], y = src[3 * (long)i + 1], z = src[3 * (long)i + 2];
        const float px = ((T[0] * x + T[1] * y) + T[2] * z) + T[9];
        const float py = ((T[3] * x + T[4] * y) + T[5] * z) + T[10];
        const float pz = ((T[6] * x + T[7] * y) + T[8] * z) + T[11];
        int cx, cy, cz;
        if (!cell_coords(px, py, pz, inv_cell, &cx, &cy, &cz)) continue;
        float best = thr2;
        for (int c = 0; c < 27; ++c) {
            const u64 key = cell_key(cx + c % 3 - 1, cy + (c / 3) % 3 - 1, cz + c / 9 - 1);
            unsigned s = __umulhi(mix32(key), tsize);
            int cnt_c = 0, start = 0;
            for (unsigned probe = 0; probe < tsize; ++probe) {
                const Slot sl = load_slot(&tab[s]);
                if (sl.key == key) { cnt_c = sl.cnt; start = sl.start; break; }
                if (sl.key == kEmptyKey) break;
                s = s + 1 == tsize ? 0 : s + 1;
            }
            for (int e = 0; e < cnt_c; ++e) {
                const float4 p = g.spts[start + e];
                const float dx = p.x - px, dy = p.y - py, dz = p.z - pz;
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                best = d2 < best ? d2 : best;
            }
        }
        if (best < thr2) { ++cnt; sum += (double)best; }
    }
    s_c[threadIdx.x] = cnt;
    s_s[threadIdx.x] = sum;
    __syncthreads();
    for (int w = kEvalThreads / 2; w >= 1; w >>= 1) {              // fixed tree: the same additions in the same order every run
        if (threadIdx.x < w) {
            s_c[threadIdx.x] += s_c[threadIdx.x + w];
            s_s[threadIdx.x] = s_s[threadIdx.x] + s_s[threadIdx.x + w];
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kEvalThreads) k_evaluate(const float* __restrict__ src, int n, GridView g, float thr2,
                                                           const int* __restrict__ npass, int max_validation,
                                                           const int* __restrict__ vid, const float* __restrict__ xf,
                                                           int* __restrict__ counts, double* __restrict__ sums,
                                                           int* __restrict__ tr_counts, double* __restrict__ tr_sums) {
    __shared__ int s_c[kEvalThreads];
    __shared__ double s_s[kEvalThreads];
    const int v = blockIdx.x;
    const int nv = min(*npass, max_validation);
    if (v >= nv) return;
    const int h = vid[v];
    evaluate_block(src, n, g, g.tab, g.hdr->ns, thr2, xf + 12 * (long)h, s_c, s_s);
    if (threadIdx.x == 0) {
        counts[v] = s_c[0];
        sums[v] = s_s[0];
        if (tr_counts) tr_counts[v] = s_c[0];
        if (tr_sums) tr_sums[v] = s_s[0];
    }
}

// ---- selection -----------------------------------------------------------------------------------------------------
__device__ inline bool better(int c1, double s1, int h1, int c2, double s2, int h2) {
    return c1 > c2 || (c1 == c2 && (s1 < s2 || (s1 == s2 && h1 < h2)));
}

// The best of the nv validated hypotheses vid[0..nv) of one pair (one workgroup of 256), re-fitted, and the statistics.
// Shared by k_select and k_select_batch.
__device__ __forceinline__ void select_block(const HypArgs& a, int n, int nv, const int* vid,
                                             const int* counts, const double* sums,
                                             double* out_t, double* out_stats) {
    __shared__ int s_c[256], s_h[256];
    __shared__ double s_s[256];
    int bc = -1, bh = 0x7FFFFFFF;
    double bs = 0.0;
    for (int v = threadIdx.x; v < nv; v += 256) {
        const int c = counts[v], h = vid[v];
        const double s = sums[v];
        if (better(c, s, h, bc, bs, bh)) { bc = c; bs = s; bh = h; }
    }
    s_c[threadIdx.x] = bc; s_s[threadIdx.x] = bs; s_h[threadIdx.x] = bh;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (threadIdx.x < w) {
            const int o = threadIdx.x + w;
            if (better(s_c[o], s_s[o], s_h[o], s_c[threadIdx.x], s_s[threadIdx.x], s_h[threadIdx.x])) {
                s_c[threadIdx.x] = s_c[o]; s_s[threadIdx.x] = s_s[o]; s_h[threadIdx.x] = s_h[o];
            }
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const int K = list_size(a);
    double T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    double fitness = 0.0, rmse = 0.0, chosen = -1.0;
    if (nv > 0 && s_c[0] > 0) {                 // a hypothesis without inliers does not beat open3d's default result
        int rows[kMaxSample];
        double R[9], t[3];
        hypothesis(a, s_h[0], K, rows, R, t);
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) T[4 * r + c] = R[3 * r + c];
            T[4 * r + 3] = t[r];
        }
        fitness = (double)s_c[0] / (double)n;
        rmse = sqrt(s_s[0] / (double)s_c[0]);
        chosen = (double)s_h[0];
    }
    for (int e = 0; e < 16; ++e) out_t[e] = T[e];
    out_stats[0] = fitness;
    out_stats[1] = rmse;
    out_stats[2] = (double)K;
    out_stats[3] = (double)a.max_iteration;
    out_stats[4] = (double)nv;
    out_stats[5] = chosen;
}

__global__ void __launch_bounds__(256) k_select(HypArgs a, int n, const int* __restrict__ npass, int max_validation,
                                                const int* __restrict__ vid, const int* __restrict__ counts,
                                                const double* __restrict__ sums, double* __restrict__ out_t,
                                                double* __restrict__ out_stats) {
    select_block(a, n, min(*npass, max_validation), vid, counts, sums, out_t, out_stats);
}

// ---- several pairs per call -----------------------------------------------------------------------------------------
// Pair p is the single-pair problem on src[src_off[p] ..], tgt[tgt_off[p] ..], corr rows from src_off[p] (local indices),
// k[p] and seeds[p]; every kernel below takes the pair from a grid dimension and runs the single-pair device code on it.
struct BatchArgs {
    const float* src;
    const int* src_off;
    const float* tgt;
    const int* tgt_off;
    const int* corr;
    const int* k;
    const u64* seeds;
    int ransac_n, dist_check, max_iteration, max_validation;
    double thr, sim;
};

__device__ inline HypArgs pair_args(const BatchArgs& b, int p) {
    const int i0 = b.src_off[p], j0 = b.tgt_off[p];
    HypArgs a;
    a.src = b.src + 3 * (long)i0; a.tgt = b.tgt + 3 * (long)j0; a.corr = b.corr + 2 * (long)i0; a.k = b.k + p;
    a.k_max = b.src_off[p + 1] - i0; a.ransac_n = b.ransac_n; a.dist_check = b.dist_check; a.max_iteration = b.max_iteration;
    a.thr = b.thr; a.sim = b.sim; a.seed = b.seeds[p];
    return a;
}

// passing hypotheses of pair p before the pair's first flag (offs = exclusive scan of all B * max_iteration flags, total =
// its grand total) -> the pair's count
__device__ inline int pair_npass(const int* offs, const int* total, int p, int B, int max_iteration) {
    const int end = p + 1 < B ? offs[(long)(p + 1) * max_iteration] : *total;
    return end - offs[(long)p * max_iteration];
}

// grid (hypothesis blocks, pair): the pass flag only; a pair with an empty target passes nothing (its corr rows point at
// target 0, which it does not have)
__global__ void __launch_bounds__(256) k_hypotheses_batch(BatchArgs b, int* __restrict__ pass) {
    const int p = blockIdx.y, h = blockIdx.x * 256 + threadIdx.x;
    if (h >= b.max_iteration) return;
    const HypArgs a = pair_args(b, p);
    int rows[kMaxSample];
    double R[9], t[3];
    const bool ok = b.tgt_off[p + 1] > b.tgt_off[p] && hypothesis(a, h, list_size(a), rows, R, t);
    pass[(long)p * b.max_iteration + h] = ok ? 1 : 0;
}

// vid[p, o] = the pair-local h of the pair's o-th passing hypothesis, o < max_validation
__global__ void __launch_bounds__(256) k_compact_batch(const int* __restrict__ pass, const int* __restrict__ offs, int max_iteration,
                                                       int max_validation, int* __restrict__ vid) {
    const int p = blockIdx.y, h = blockIdx.x * 256 + threadIdx.x;
    const long g = (long)p * max_iteration + h;
    if (h >= max_iteration || !pass[g]) return;
    const int o = offs[g] - offs[(long)p * max_iteration];
    if (o < max_validation) vid[(long)p * max_validation + o] = h;
}

// the fp32 R|t of the validated hypotheses only (the single-pair path keeps it for every hypothesis): hypothesis() is
// deterministic, so the refit is the same bits as the fit of k_hypotheses_batch
__global__ void __launch_bounds__(256) k_refit_batch(BatchArgs b, const int* __restrict__ offs, const int* __restrict__ total, int B,
                                                     const int* __restrict__ vid, float* __restrict__ xf) {
    const int p = blockIdx.y, v = blockIdx.x * 256 + threadIdx.x;
    if (v >= min(pair_npass(offs, total, p, B, b.max_iteration), b.max_validation)) return;
    const long slot = (long)p * b.max_validation + v;
    const HypArgs a = pair_args(b, p);
    int rows[kMaxSample];
    double R[9], t[3];
    hypothesis(a, vid[slot], list_size(a), rows, R, t);
    for (int e = 0; e < 9; ++e) xf[12 * slot + e] = (float)R[e];
    for (int e = 0; e < 3; ++e) xf[12 * slot + 9 + e] = (float)t[e];
}

// grid (validated hypothesis, pair); pair p's table in the grid over all targets is the 2 m_p slots at 2 tgt_off[p]
__global__ void __launch_bounds__(kEvalThreads) k_evaluate_batch(BatchArgs b, GridView g, float thr2, const int* __restrict__ offs,
                                                                 const int* __restrict__ total, int B, const float* __restrict__ xf,
                                                                 int* __restrict__ counts, double* __restrict__ sums) {
    __shared__ int s_c[kEvalThreads];
    __shared__ double s_s[kEvalThreads];
    const int p = blockIdx.y, v = blockIdx.x;
    if (v >= min(pair_npass(offs, total, p, B, b.max_iteration), b.max_validation)) return;
    const long slot = (long)p * b.max_validation + v;
    const int i0 = b.src_off[p], j0 = b.tgt_off[p];
    evaluate_block(b.src + 3 * (long)i0, b.src_off[p + 1] - i0, g, g.tab + 2 * (long)j0, b.tgt_off[p + 1] - j0, thr2,
                   xf + 12 * slot, s_c, s_s);
    if (threadIdx.x == 0) {
        counts[slot] = s_c[0];
        sums[slot] = s_s[0];
    }
}

// one workgroup per pair; a seed >= 2^24 (not checkable on the host: seeds live on the device) gives NaN outputs
__global__ void __launch_bounds__(256) k_select_batch(BatchArgs b, const int* __restrict__ offs, const int* __restrict__ total, int B,
                                                      const int* __restrict__ vid, const int* __restrict__ counts,
                                                      const double* __restrict__ sums, double* __restrict__ out_t,
                                                      double* __restrict__ out_stats) {
    const int p = blockIdx.x;
    if (b.seeds[p] >= (1ull << 24)) {
        if (threadIdx.x < 16) out_t[16 * (long)p + threadIdx.x] = __builtin_nan("");
        if (threadIdx.x < 6) out_stats[6 * (long)p + threadIdx.x] = __builtin_nan("");
        return;
    }
    const long base = (long)p * b.max_validation;
    select_block(pair_args(b, p), b.src_off[p + 1] - b.src_off[p],
                 min(pair_npass(offs, total, p, B, b.max_iteration), b.max_validation), vid + base, counts + base, sums + base,
                 out_t + 16 * (long)p, out_stats + 6 * (long)p);
}

struct RansacWs {
    int* pass;
    int* offs;
    int* npass;
    int* vid;
    float* xf;
    int* counts;
    double* sums;
    void* scan;
};

RansacWs carve_ransac(Carver& cv, int max_iteration, int max_validation) {
    RansacWs w;
    w.pass = cv.take<int>((size_t)max_iteration);
    w.offs = cv.take<int>((size_t)max_iteration);
    w.npass = cv.take<int>(1);
    w.vid = cv.take<int>((size_t)max_validation);
    w.xf = cv.take<float>((size_t)max_iteration * 12);
    w.counts = cv.take<int>((size_t)max_validation);
    w.sums = cv.take<double>((size_t)max_validation);
    w.scan = cv.take<char>(scan_ws_bytes(max_iteration));
    return w;
}

struct MatchWs {
    u64* packed;       // [n]  (also pcrcg_feature_argmax's workspace)
    float* hb;         // [m]
    long long* arg_s;  // [n]
    long long* arg_t;  // [m]
    int* flags;        // [n]
    int* offs;         // [n]
    void* scan;
};

MatchWs carve_match(Carver& cv, int n, int m) {
    MatchWs w;
    const int nm = n > m ? n : m;
    w.packed = cv.take<u64>((size_t)(nm > 0 ? nm : 1));
    w.hb = cv.take<float>((size_t)(m > 0 ? m : 1));
    w.arg_s = cv.take<long long>((size_t)(n > 0 ? n : 1));
    w.arg_t = cv.take<long long>((size_t)(m > 0 ? m : 1));
    w.flags = cv.take<int>((size_t)(n > 0 ? n : 1));
    w.offs = cv.take<int>((size_t)(n > 0 ? n : 1));
    w.scan = cv.take<char>(scan_ws_bytes(n));
    return w;
}

// Batch workspace: the match stage and the RANSAC stage reuse the same bytes (as in the single-pair path).
struct BatchWs {
    u64* packed;   // [n_total]
    float* hb;     // [m_total]
    int* pass;     // [B * max_iteration]
    int* offs;     // [B * max_iteration]
    int* npass;    // [1]  grand total of the scan
    int* vid;      // [B * max_validation]
    float* xf;     // [B * max_validation * 12]
    int* counts;   // [B * max_validation]
    double* sums;  // [B * max_validation]
    void* scan;
};

void carve_batch_match(Carver& cv, BatchWs& w, int n_total, int m_total) {
    w.packed = cv.take<u64>((size_t)(n_total > 0 ? n_total : 1));
    w.hb = cv.take<float>((size_t)(m_total > 0 ? m_total : 1));
}

void carve_batch_ransac(Carver& cv, BatchWs& w, int B, int max_iteration, int max_validation) {
    const size_t hi = (size_t)B * (size_t)max_iteration, hv = (size_t)B * (size_t)max_validation;
    w.pass = cv.take<int>(hi);
    w.offs = cv.take<int>(hi);
    w.npass = cv.take<int>(1);
    w.vid = cv.take<int>(hv);
    w.xf = cv.take<float>(hv * 12);
    w.counts = cv.take<int>(hv);
    w.sums = cv.take<double>(hv);
    w.scan = cv.take<char>(scan_ws_bytes((int)hi));
}

// ---- inlier statistics of many pairs (pcrcg_inlier_stats_batch) ----------------------------------------------------
// Both arg-max directions of <a_i, b_j> for every pair, then one pass over every source row: the ground-truth distance of
// the row's match and the threshold counts.  The arg-max kernels run the bodies of pcrcg_feature_argmax (argmax.h) on
// the pair p = blockIdx.z (rows a_off[p] .., columns b_off[p] .., indices local to the pair); a workgroup that lies past
// its pair's rows or columns leaves at once (the whole workgroup: the VALU body synchronises).
template <int C>
__global__ void __launch_bounds__(256) k_feature_argmax_batch(const float* __restrict__ a, int lda, const int* __restrict__ a_off,
                                                              const float* __restrict__ b, int ldb, const int* __restrict__ b_off,
                                                              int cols_per, u64* __restrict__ packed) {
    __shared__ __attribute__((aligned(16))) float bs[kArgmaxTB * C];
    const int p = blockIdx.z;
    const int i0 = a_off[p], j0 = b_off[p];
    const int n = a_off[p + 1] - i0, m = b_off[p + 1] - j0;
    if ((int)blockIdx.x * 256 >= n || (int)blockIdx.y * cols_per >= m) return;
    feature_argmax_valu_tile<C>(a + (long)i0 * lda, lda, n, b + (long)j0 * ldb, ldb, m, cols_per, packed + i0, bs, blockIdx.x,
                                blockIdx.y);
}

__global__ void __launch_bounds__(256) k_feature_argmax_mfma32_batch(const float* __restrict__ a, int lda,
                                                                     const int* __restrict__ a_off, const float* __restrict__ b,
                                                                     int ldb, const int* __restrict__ b_off, int cols_per,
                                                                     u64* __restrict__ packed) {
    const int p = blockIdx.z;
    const int i0 = a_off[p], j0 = b_off[p];
    feature_argmax_mfma32_tile(a + (long)i0 * lda, lda, a_off[p + 1] - i0, b + (long)j0 * ldb, ldb, b_off[p + 1] - j0, cols_per,
                               packed + i0, blockIdx.x, blockIdx.y);
}

__global__ void __launch_bounds__(256) k_feature_argmax_any_batch(const float* __restrict__ a, int lda, const int* __restrict__ a_off,
                                                                  const float* __restrict__ b, int ldb, const int* __restrict__ b_off,
                                                                  int c, int cols_per, u64* __restrict__ packed) {
    const int p = blockIdx.z;
    const int i0 = a_off[p], j0 = b_off[p];
    feature_argmax_any_row(a + (long)i0 * lda, lda, a_off[p + 1] - i0, b + (long)j0 * ldb, ldb, b_off[p + 1] - j0, c, cols_per,
                           packed + i0, blockIdx.x * 256 + threadIdx.x, blockIdx.y);
}

// packed winners -> pair-local int32 columns, over all rows of all pairs at once
__global__ void __launch_bounds__(256) k_packed_cols(const u64* __restrict__ packed, int n, int* __restrict__ arg) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) arg[i] = packed_col(packed[i]);
}

// pcrcg_feature_argmax's launch shapes with the pair count folded into the workgroup target (the arg-max does not depend
// on how the columns are split): packed [n_total] receives the winners of every row of A against its pair's rows of B
int feature_argmax_batch(const float* a, int lda, const int* a_off, int n_total, int n_max, const float* b, int ldb,
                         const int* b_off, int m_max, int c, int B, u64* packed, hipStream_t st) {
    PCRCG_CHECK_HIP(hipMemsetAsync(packed, 0, (size_t)n_total * 8, st));
    if (c == 32 && lda % 4 == 0 && ldb % 4 == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0 &&
        debug_opts().bwd_mfma) {
        const int gxm = (n_max + 127) / 128;
        long splits = (1024 + (long)gxm * B - 1) / ((long)gxm * B);
        const int max_splits = (m_max + 255) / 256;
        if (splits > max_splits) splits = max_splits;
        if (splits < 1) splits = 1;
        const int cols_per = ((m_max + (int)splits - 1) / (int)splits + 31) / 32 * 32;
        hipLaunchKernelGGL(k_feature_argmax_mfma32_batch, dim3(gxm, (m_max + cols_per - 1) / cols_per, B), dim3(256), 0, st, a, lda,
                           a_off, b, ldb, b_off, cols_per, packed);
        PCRCG_CHECK_LAUNCH();
        return PCRCG_OK;
    }
    const int gx = (n_max + 255) / 256;
    long splits = (2048 + (long)gx * B - 1) / ((long)gx * B);
    const int max_splits = (m_max + 127) / 128;
    if (splits > max_splits) splits = max_splits;
    if (splits < 1) splits = 1;
    const int cols_per = ((m_max + (int)splits - 1) / (int)splits + 127) / 128 * 128;
    const dim3 grid(gx, (m_max + cols_per - 1) / cols_per, B);
    if (c == 32) hipLaunchKernelGGL(k_feature_argmax_batch<32>, grid, dim3(256), 0, st, a, lda, a_off, b, ldb, b_off, cols_per, packed);
    else if (c == 64) hipLaunchKernelGGL(k_feature_argmax_batch<64>, grid, dim3(256), 0, st, a, lda, a_off, b, ldb, b_off, cols_per, packed);
    else hipLaunchKernelGGL(k_feature_argmax_any_batch, grid, dim3(256), 0, st, a, lda, a_off, b, ldb, b_off, c, cols_per, packed);
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}

constexpr int kMaxThresholds = 32;

struct InlierArgs {
    const float* src;
    const int* src_off;
    const float* tgt;
    const int* tgt_off;
    const u64* ps;      // [n_total] winners of the source rows (column = target, local)
    const u64* pt;      // [m_total] winners of the target rows (column = source, local)
    const float* rt;    // [B, 12] R (row-major) then t
    int* counts;        // [B, 2, n_thr]: "wo" then "w"
    int* k_mutual;      // [B]
    float* dist;        // [n_total] or null
    int* mutual;        // [n_total] or null
    int n_thr;
    float thr[kMaxThresholds];
};

// grid (row blocks, pair): one thread per source row i of pair p.  The row's match j = arg_s[i] (local), the source point
// moved with unfused fp32 ((r0 x + r1 y) + r2 z) + t (the arithmetic of RANSAC's evaluation), d = sqrtf(((dx dx + dy dy) +
// dz dz)) correctly rounded (this file is compiled without contraction and with HIP's correctly rounded fp32 sqrt), and
// for every threshold "wo" += d < thr, "w" += (arg_t[j] == i) && d < thr.  Integer counts: the workgroup's wavefronts
// meet by ballots in LDS and the workgroups by atomicAdd, so the totals do not depend on the order.
__global__ void __launch_bounds__(256) k_inlier_stats(InlierArgs s) {
    __shared__ int s_cnt[2 * kMaxThresholds + 1];
    __shared__ float s_thr[kMaxThresholds];
    const int p = blockIdx.y;
    const int i0 = s.src_off[p], n = s.src_off[p + 1] - i0;
    const int j0 = s.tgt_off[p], m = s.tgt_off[p + 1] - j0;
    if ((int)blockIdx.x * 256 >= n) return;
    const int nt = s.n_thr;
    if (threadIdx.x < 2 * nt + 1) s_cnt[threadIdx.x] = 0;
    if (threadIdx.x < nt) s_thr[threadIdx.x] = s.thr[threadIdx.x];
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    float d = __builtin_nanf("");
    bool live = false, mut = false;
    if (i < n) {
        const int j = packed_col(s.ps[i0 + i]);
        if (j >= 0 && j < m) {                       // always, unless the pair has no target (m = 0): no match, NaN
            live = true;
            const float* T = s.rt + 12 * (long)p;
            const float* q = s.src + 3 * (long)(i0 + i);
            const float* t = s.tgt + 3 * (long)(j0 + j);
            const float x = q[0], y = q[1], z = q[2];
            const float px = ((T[0] * x + T[1] * y) + T[2] * z) + T[9];
            const float py = ((T[3] * x + T[4] * y) + T[5] * z) + T[10];
            const float pz = ((T[6] * x + T[7] * y) + T[8] * z) + T[11];
            const float dx = px - t[0], dy = py - t[1], dz = pz - t[2];
            d = sqrtf((dx * dx + dy * dy) + dz * dz);
            mut = packed_col(s.pt[j0 + j]) == i;
        }
        if (s.dist) s.dist[i0 + i] = d;
        if (s.mutual) s.mutual[i0 + i] = mut ? 1 : 0;
    }
    const bool lane0 = (threadIdx.x & 63) == 0;
    const u64 km = __ballot(live && mut);
    if (lane0 && km) atomicAdd(&s_cnt[2 * nt], (int)__popcll(km));
    for (int k = 0; k < nt; ++k) {
        const bool in = live && d < s_thr[k];
        const u64 wo = __ballot(in), w = __ballot(in && mut);
        if (lane0 && wo) atomicAdd(&s_cnt[k], (int)__popcll(wo));
        if (lane0 && w) atomicAdd(&s_cnt[nt + k], (int)__popcll(w));
    }
    __syncthreads();
    if (threadIdx.x < 2 * nt && s_cnt[threadIdx.x]) atomicAdd(&s.counts[2 * nt * (long)p + threadIdx.x], s_cnt[threadIdx.x]);
    if (threadIdx.x == 2 * nt && s_cnt[2 * nt]) atomicAdd(&s.k_mutual[p], s_cnt[2 * nt]);
}

struct InlierWs {
    u64* ps;   // [n_total]
    u64* pt;   // [m_total]
};

InlierWs carve_inlier(Carver& cv, int n_total, int m_total) {
    InlierWs w;
    w.ps = cv.take<u64>((size_t)(n_total > 0 ? n_total : 1));
    w.pt = cv.take<u64>((size_t)(m_total > 0 ? m_total : 1));
    return w;
}

constexpr int kMaxBatch = 65535;      // pairs ride on a grid dimension

// The L2 arg-max of every row of a over its pair's rows of b, for B ragged pairs (pcrcg_feature_match_batch; both directions of
// pcrcg_mutual_match_batch): packed [rows of a] must be zeroed, hb = k_half_norms of b.  The single-pair launch shapes with the
// pair count folded into the workgroup target; the arg-max does not depend on how the columns are split, so every pair gets
// the single-pair result.
void launch_l2nn_batch(const float* a, int lda, const int* a_off, int n_max, const float* b, int ldb, const int* b_off, int m_max,
                       int c, int B, const float* hb, u64* packed, hipStream_t st) {
    const bool aligned = lda % 4 == 0 && ldb % 4 == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0;
    if ((c == 32 || c == 64) && aligned) {
        const int gxm = (n_max + 127) / 128;
        long splits = (1024 + (long)gxm * B - 1) / ((long)gxm * B);
        const int max_splits = (m_max + 255) / 256;
        if (splits > max_splits) splits = max_splits;
        if (splits < 1) splits = 1;
        const int cols_per = ((m_max + (int)splits - 1) / (int)splits + 31) / 32 * 32;
        const dim3 grid(gxm, (m_max + cols_per - 1) / cols_per, B);
        if (c == 32)
            hipLaunchKernelGGL(k_l2nn_mfma_batch<32>, grid, dim3(256), 0, st, a, lda, a_off, b, ldb, b_off, hb, cols_per, packed);
        else
            hipLaunchKernelGGL(k_l2nn_mfma_batch<64>, grid, dim3(256), 0, st, a, lda, a_off, b, ldb, b_off, hb, cols_per, packed);
    } else {
        const int gx = (n_max + 255) / 256;
        long splits = (2048 + (long)gx * B - 1) / ((long)gx * B);
        const int max_splits = (m_max + 127) / 128;
        if (splits > max_splits) splits = max_splits;
        if (splits < 1) splits = 1;
        const int cols_per = (m_max + (int)splits - 1) / (int)splits;
        hipLaunchKernelGGL(k_l2nn_any_batch, dim3(gx, (m_max + cols_per - 1) / cols_per, B), dim3(256), 0, st, a, lda, a_off, b,
                           ldb, b_off, c, hb, cols_per, packed);
    }
}

struct MutualWs {
    u64* ps;       // [n_total] the rows' arg-max words
    u64* pt;       // [m_total] the columns'
    float* hs;     // [n_total] |a_i|^2 / 2
    float* ht;     // [m_total] |b_j|^2 / 2
};

MutualWs carve_mutual(Carver& cv, int n_total, int m_total) {
    MutualWs w;
    w.ps = cv.take<u64>((size_t)(n_total > 0 ? n_total : 1));
    w.pt = cv.take<u64>((size_t)(m_total > 0 ? m_total : 1));
    w.hs = cv.take<float>((size_t)(n_total > 0 ? n_total : 1));
    w.ht = cv.take<float>((size_t)(m_total > 0 ? m_total : 1));
    return w;
}

}  // namespace
}  // namespace pcrcg

using namespace pcrcg;

extern "C" {

size_t pcrcg_ransac_ws_bytes(int n, int m, int max_iteration, int max_validation) {
    if (n < 0 || m < 0 || max_iteration < 0 || max_validation < 0) return 0;
    Carver a(nullptr, 0), b(nullptr, 0);
    carve_match(a, n, m);
    carve_ransac(b, max_iteration > 0 ? max_iteration : 1, max_validation > 0 ? max_validation : 1);
    return a.off > b.off ? a.off : b.off;
}

int pcrcg_feature_match(const float* src_feat, int ld_src, int n, const float* tgt_feat, int ld_tgt, int m, int c, int mutual,
                        int* corr, int* k, void* ws, size_t ws_bytes, void* stream) {
    PCRCG_CHECK_ARG(src_feat && tgt_feat && corr && k && ws);
    PCRCG_CHECK_ARG(n >= 1 && m >= 1 && c >= 1 && ld_src >= c && ld_tgt >= c);
    PCRCG_CHECK_ARG(mutual == 0 || mutual == 1);
    Carver cv(ws, ws_bytes);
    MatchWs w = carve_match(cv, n, m);
    PCRCG_CHECK_WS(cv);
    hipStream_t st = as_stream(stream);
    const int gx = (n + 255) / 256;
    if (mutual) {
        const size_t abytes = carve_bytes((size_t)(n > m ? n : m), 8);
        PCRCG_PROPAGATE(pcrcg_feature_argmax(src_feat, ld_src, n, tgt_feat, ld_tgt, m, c,
                                             reinterpret_cast<int64_t*>(w.arg_s), nullptr, w.packed, abytes, stream));
        PCRCG_PROPAGATE(pcrcg_feature_argmax(tgt_feat, ld_tgt, m, src_feat, ld_src, n, c,
                                             reinterpret_cast<int64_t*>(w.arg_t), nullptr, w.packed, abytes, stream));
        hipLaunchKernelGGL(k_mutual_flags, dim3(gx), dim3(256), 0, st, w.arg_s, n, w.arg_t, w.flags);
        PCRCG_CHECK_LAUNCH();
        PCRCG_PROPAGATE(exclusive_scan_i32(w.flags, w.offs, n, k, w.scan, st));
        hipLaunchKernelGGL(k_mutual_emit, dim3(gx), dim3(256), 0, st, w.flags, w.offs, n, w.arg_s, corr);
        PCRCG_CHECK_LAUNCH();
        return PCRCG_OK;
    }
    PCRCG_CHECK_HIP(hipMemsetAsync(w.packed, 0, (size_t)n * 8, st));
    hipLaunchKernelGGL(k_half_norms, dim3((m + 255) / 256), dim3(256), 0, st, tgt_feat, ld_tgt, m, c, w.hb);
    const bool aligned = ld_src % 4 == 0 && ld_tgt % 4 == 0 &&
                         ((reinterpret_cast<uintptr_t>(src_feat) | reinterpret_cast<uintptr_t>(tgt_feat)) & 15) == 0;
    if ((c == 32 || c == 64) && aligned) {
        const int gxm = (n + 127) / 128;               // 128 rows per workgroup, column ranges for ~1k workgroups in flight
        int splits = (1024 + gxm - 1) / gxm;
        const int max_splits = (m + 255) / 256;
        if (splits > max_splits) splits = max_splits;
        if (splits < 1) splits = 1;
        const int cols_per = ((m + splits - 1) / splits + 31) / 32 * 32;
        const dim3 grid(gxm, (m + cols_per - 1) / cols_per);
        if (c == 32)
            hipLaunchKernelGGL(k_l2nn_mfma<32>, grid, dim3(256), 0, st, src_feat, ld_src, n, tgt_feat, ld_tgt, m, w.hb, cols_per,
                               w.packed);
        else
            hipLaunchKernelGGL(k_l2nn_mfma<64>, grid, dim3(256), 0, st, src_feat, ld_src, n, tgt_feat, ld_tgt, m, w.hb, cols_per,
                               w.packed);
    } else {
        int splits = (2048 + gx - 1) / gx;
        const int max_splits = (m + 127) / 128;
        if (splits > max_splits) splits = max_splits;
        if (splits < 1) splits = 1;
        const int cols_per = (m + splits - 1) / splits;
        hipLaunchKernelGGL(k_l2nn_any, dim3(gx, (m + cols_per - 1) / cols_per), dim3(256), 0, st, src_feat, ld_src, n, tgt_feat,
                           ld_tgt, m, c, w.hb, cols_per, w.packed);
    }
    hipLaunchKernelGGL(k_nn_emit, dim3(gx), dim3(256), 0, st, w.packed, n, corr, k);
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}

int pcrcg_ransac(const float* src, int n, const float* tgt, int m, const void* grid, const int* corr, int k_max, const int* k,
                 int ransac_n, double threshold, double edge_similarity, int distance_check, int max_iteration,
                 int max_validation, uint64_t seed, double* out_transform, double* out_stats, const pcrcg_ransac_trace* trace,
                 void* ws, size_t ws_bytes, void* stream) {
    PCRCG_CHECK_ARG(src && tgt && grid && corr && k && out_transform && out_stats && ws);
    PCRCG_CHECK_ARG(n >= 1 && m >= 1 && k_max >= 0);
    PCRCG_CHECK_ARG(ransac_n >= 3 && ransac_n <= kMaxSample);
    PCRCG_CHECK_ARG(k_max >= ransac_n);
    PCRCG_CHECK_ARG(threshold > 0.0 && edge_similarity >= 0.0 && edge_similarity <= 1.0);
    PCRCG_CHECK_ARG(distance_check == 0 || distance_check == 1);
    PCRCG_CHECK_ARG(max_iteration >= 1 && max_iteration <= (1 << 27));
    PCRCG_CHECK_ARG(max_validation >= 1 && max_validation <= max_iteration);
    PCRCG_CHECK_ARG(seed < (1ull << 24));
    Carver cv(ws, ws_bytes);
    RansacWs w = carve_ransac(cv, max_iteration, max_validation);
    PCRCG_CHECK_WS(cv);
    bool ok;
    GridView g = grid_view(const_cast<void*>(grid), grid_bytes(m, 1), m, 1, &ok);
    hipStream_t st = as_stream(stream);
    pcrcg_ransac_trace tr = {};
    if (trace) tr = *trace;
    HypArgs a;
    a.src = src; a.tgt = tgt; a.corr = corr; a.k = k;
    a.k_max = k_max; a.ransac_n = ransac_n; a.dist_check = distance_check; a.max_iteration = max_iteration;
    a.thr = threshold; a.sim = edge_similarity; a.seed = seed;
    const int gh = (max_iteration + 255) / 256;
    hipLaunchKernelGGL(k_hypotheses, dim3(gh), dim3(256), 0, st, a, w.pass, w.xf, tr.samples, tr.pass, tr.xf32, tr.xf64);
    PCRCG_CHECK_LAUNCH();
    PCRCG_PROPAGATE(exclusive_scan_i32(w.pass, w.offs, max_iteration, w.npass, w.scan, st));
    hipLaunchKernelGGL(k_compact, dim3(gh), dim3(256), 0, st, w.pass, w.offs, max_iteration, max_validation, w.vid, tr.valid_ids);
    const float thr2 = (float)(threshold * threshold);
    hipLaunchKernelGGL(k_evaluate, dim3(max_validation), dim3(kEvalThreads), 0, st, src, n, g, thr2, w.npass, max_validation, w.vid,
                       w.xf, w.counts, w.sums, tr.counts, tr.sums);
    hipLaunchKernelGGL(k_select, dim3(1), dim3(256), 0, st, a, n, w.npass, max_validation, w.vid, w.counts, w.sums, out_transform,
                       out_stats);
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}

size_t pcrcg_ransac_batch_ws_bytes(int B, int n_total, int m_total, int max_iteration, int max_validation) {
    if (B < 1 || B > kMaxBatch || n_total < 0 || m_total < 0 || max_iteration < 1 || max_validation < 1) return 0;
    if ((long long)B * max_iteration > 0x7FFFFFFF) return 0;
    Carver a(nullptr, 0), b(nullptr, 0);
    BatchWs w;
    carve_batch_match(a, w, n_total, m_total);
    carve_batch_ransac(b, w, B, max_iteration, max_validation);
    return a.off > b.off ? a.off : b.off;
}

int pcrcg_feature_match_batch(const float* src_feat, int ld_src, const int* src_off, int n_total, int n_max,
                              const float* tgt_feat, int ld_tgt, const int* tgt_off, int m_total, int m_max, int c, int B,
                              int* corr, int* k, void* ws, size_t ws_bytes, void* stream) {
    PCRCG_CHECK_ARG(src_feat && src_off && tgt_feat && tgt_off && corr && k && ws);
    PCRCG_CHECK_ARG(B >= 1 && B <= kMaxBatch);
    PCRCG_CHECK_ARG(n_max >= 1 && m_max >= 1 && n_total >= n_max && m_total >= m_max);
    PCRCG_CHECK_ARG(c >= 1 && ld_src >= c && ld_tgt >= c);
    Carver cv(ws, ws_bytes);
    BatchWs w;
    carve_batch_match(cv, w, n_total, m_total);
    PCRCG_CHECK_WS(cv);
    hipStream_t st = as_stream(stream);
    PCRCG_CHECK_HIP(hipMemsetAsync(w.packed, 0, (size_t)n_total * 8, st));
    hipLaunchKernelGGL(k_half_norms, dim3((m_total + 255) / 256), dim3(256), 0, st, tgt_feat, ld_tgt, m_total, c, w.hb);
    launch_l2nn_batch(src_feat, ld_src, src_off, n_max, tgt_feat, ld_tgt, tgt_off, m_max, c, B, w.hb, w.packed, st);
    hipLaunchKernelGGL(k_nn_emit_batch, dim3((n_max + 255) / 256, B), dim3(256), 0, st, w.packed, src_off, corr, k);
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}

size_t pcrcg_mutual_match_batch_ws_bytes(int B, int n_total, int m_total) {
    if (B < 1 || B > kMaxBatch || n_total < 0 || m_total < 0) return 0;
    Carver cv(nullptr, 0);
    carve_mutual(cv, n_total, m_total);
    return cv.off;
}

int pcrcg_mutual_match_batch(const float* src_feat, int ld_src, const int* src_off, int n_total, int n_max,
                             const float* tgt_feat, int ld_tgt, const int* tgt_off, int m_total, int m_max, int c, int B,
                             int* corr, int* k, void* ws, size_t ws_bytes, void* stream) {
    PCRCG_CHECK_ARG(src_feat && src_off && tgt_feat && tgt_off && corr && k && ws);
    PCRCG_CHECK_ARG(B >= 1 && B <= kMaxBatch);
    PCRCG_CHECK_ARG(n_max >= 1 && m_max >= 1 && n_total >= n_max && m_total >= m_max);
    PCRCG_CHECK_ARG(c >= 1 && ld_src >= c && ld_tgt >= c);
    Carver cv(ws, ws_bytes);
    MutualWs w = carve_mutual(cv, n_total, m_total);
    PCRCG_CHECK_WS(cv);
    hipStream_t st = as_stream(stream);
    PCRCG_CHECK_HIP(hipMemsetAsync(w.ps, 0, (size_t)n_total * 8, st));
    PCRCG_CHECK_HIP(hipMemsetAsync(w.pt, 0, (size_t)m_total * 8, st));
    hipLaunchKernelGGL(k_half_norms, dim3((m_total + 255) / 256), dim3(256), 0, st, tgt_feat, ld_tgt, m_total, c, w.ht);
    hipLaunchKernelGGL(k_half_norms, dim3((n_total + 255) / 256), dim3(256), 0, st, src_feat, ld_src, n_total, c, w.hs);
    // nn_s: pcrcg_feature_match_batch's launch; nn_t: the same with the roles exchanged
    launch_l2nn_batch(src_feat, ld_src, src_off, n_max, tgt_feat, ld_tgt, tgt_off, m_max, c, B, w.ht, w.ps, st);
    launch_l2nn_batch(tgt_feat, ld_tgt, tgt_off, m_max, src_feat, ld_src, src_off, n_max, c, B, w.hs, w.pt, st);
    hipLaunchKernelGGL(k_mutual_emit_batch, dim3(B), dim3(256), 0, st, w.ps, src_off, w.pt, tgt_off, corr, k);
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}

int pcrcg_ransac_batch(const float* src, const int* src_off, const float* tgt, const int* tgt_off, int m_total, const void* grid, const int* corr, const int* k, int B, int ransac_n, double threshold,
                       double edge_similarity, int distance_check, int max_iteration, int max_validation,
                       const uint64_t* seeds, double* out_transform, double* out_stats, void* ws, size_t ws_bytes,
                       void* stream) {
    PCRCG_CHECK_ARG(src && src_off && tgt && tgt_off && grid && corr && k && seeds && out_transform && out_stats && ws);
    PCRCG_CHECK_ARG(B >= 1 && B <= kMaxBatch);
    PCRCG_CHECK_ARG(ransac_n >= 3 && ransac_n <= kMaxSample);
    PCRCG_CHECK_ARG(m_total >= 1);
    PCRCG_CHECK_ARG(threshold > 0.0 && edge_similarity >= 0.0 && edge_similarity <= 1.0);
    PCRCG_CHECK_ARG(distance_check == 0 || distance_check == 1);
    PCRCG_CHECK_ARG(max_iteration >= 1 && max_iteration <= (1 << 27));
    PCRCG_CHECK_ARG(max_validation >= 1 && max_validation <= max_iteration);
    PCRCG_CHECK_ARG((long long)B * max_iteration <= 0x7FFFFFFF);
    Carver cv(ws, ws_bytes);
    BatchWs w;
    carve_batch_ransac(cv, w, B, max_iteration, max_validation);
    PCRCG_CHECK_WS(cv);
    bool ok;
    GridView g = grid_view(const_cast<void*>(grid), grid_bytes(m_total, B), m_total, B, &ok);
    hipStream_t st = as_stream(stream);
    BatchArgs a;
    a.src = src; a.src_off = src_off; a.tgt = tgt; a.tgt_off = tgt_off; a.corr = corr; a.k = k;
    a.seeds = reinterpret_cast<const u64*>(seeds);
    a.ransac_n = ransac_n; a.dist_check = distance_check; a.max_iteration = max_iteration; a.max_validation = max_validation;
    a.thr = threshold; a.sim = edge_similarity;
    const int gh = (max_iteration + 255) / 256;
    hipLaunchKernelGGL(k_hypotheses_batch, dim3(gh, B), dim3(256), 0, st, a, w.pass);
    PCRCG_CHECK_LAUNCH();
    PCRCG_PROPAGATE(exclusive_scan_i32(w.pass, w.offs, B * max_iteration, w.npass, w.scan, st));
    hipLaunchKernelGGL(k_compact_batch, dim3(gh, B), dim3(256), 0, st, w.pass, w.offs, max_iteration, max_validation, w.vid);
    hipLaunchKernelGGL(k_refit_batch, dim3((max_validation + 255) / 256, B), dim3(256), 0, st, a, w.offs, w.npass, B, w.vid, w.xf);
    const float thr2 = (float)(threshold * threshold);
    hipLaunchKernelGGL(k_evaluate_batch, dim3(max_validation, B), dim3(kEvalThreads), 0, st, a, g, thr2, w.offs, w.npass, B, w.xf,
                       w.counts, w.sums);
    hipLaunchKernelGGL(k_select_batch, dim3(B), dim3(256), 0, st, a, w.offs, w.npass, B, w.vid, w.counts, w.sums, out_transform,
                       out_stats);
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}

size_t pcrcg_inlier_stats_batch_ws_bytes(int B, int n_total, int m_total) {
    if (B < 1 || B > kMaxBatch || n_total < 1 || m_total < 1) return 0;
    Carver cv(nullptr, 0);
    carve_inlier(cv, n_total, m_total);
    return cv.off;
}

int pcrcg_inlier_stats_batch(const float* src, const float* src_feat, int ld_src, const int* src_off, int n_total, int n_max,
                             const float* tgt, const float* tgt_feat, int ld_tgt, const int* tgt_off, int m_total, int m_max,
                             int c, int B, const float* rt, const float* thr, int n_thr, int* counts, int* k_mutual,
                             float* dist, int* mutual, int* arg_s, int* arg_t, void* ws, size_t ws_bytes, void* stream) {
    PCRCG_CHECK_ARG(src && src_feat && src_off && tgt && tgt_feat && tgt_off && rt && thr && counts && k_mutual && ws);
    PCRCG_CHECK_ARG(B >= 1 && B <= kMaxBatch);
    PCRCG_CHECK_ARG(n_thr >= 1 && n_thr <= kMaxThresholds);
    PCRCG_CHECK_ARG(n_max >= 1 && m_max >= 1 && n_total >= n_max && m_total >= m_max);
    PCRCG_CHECK_ARG(c >= 1 && ld_src >= c && ld_tgt >= c);
    Carver cv(ws, ws_bytes);
    InlierWs w = carve_inlier(cv, n_total, m_total);
    PCRCG_CHECK_WS(cv);
    InlierArgs a;
    for (int k = 0; k < n_thr; ++k) {
        PCRCG_CHECK_ARG(!(thr[k] != thr[k]));        // a NaN threshold
        a.thr[k] = thr[k];
    }
    for (int k = n_thr; k < kMaxThresholds; ++k) a.thr[k] = 0.f;
    hipStream_t st = as_stream(stream);
    PCRCG_PROPAGATE(feature_argmax_batch(src_feat, ld_src, src_off, n_total, n_max, tgt_feat, ld_tgt, tgt_off, m_max, c, B, w.ps, st));
    PCRCG_PROPAGATE(feature_argmax_batch(tgt_feat, ld_tgt, tgt_off, m_total, m_max, src_feat, ld_src, src_off, n_max, c, B, w.pt, st));
    PCRCG_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)B * 2 * n_thr * sizeof(int), st));
    PCRCG_CHECK_HIP(hipMemsetAsync(k_mutual, 0, (size_t)B * sizeof(int), st));
    a.src = src; a.src_off = src_off; a.tgt = tgt; a.tgt_off = tgt_off; a.ps = w.ps; a.pt = w.pt; a.rt = rt;
    a.counts = counts; a.k_mutual = k_mutual; a.dist = dist; a.mutual = mutual; a.n_thr = n_thr;
    hipLaunchKernelGGL(k_inlier_stats, dim3((n_max + 255) / 256, B), dim3(256), 0, st, a);
    PCRCG_CHECK_LAUNCH();
    if (arg_s) hipLaunchKernelGGL(k_packed_cols, dim3((n_total + 255) / 256), dim3(256), 0, st, w.ps, n_total, arg_s);
    if (arg_t) hipLaunchKernelGGL(k_packed_cols, dim3((m_total + 255) / 256), dim3(256), 0, st, w.pt, m_total, arg_t);
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}

}  // extern "C"
