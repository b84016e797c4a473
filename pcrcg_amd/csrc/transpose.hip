// transpose.hip -- neighbour tables transposed once per pyramid, and the backward passes that GATHER over them instead of
// scattering with atomics (include/pcrcg_train.h: pcrcg_neighbors_transpose_*, pcrcg_kpconv_backward_dx_t,
// pcrcg_gather_max_backward_t, pcrcg_gather_first_backward_t).
//
// A table idx [nq, h] lists, per query, the supports it reads.  Its transpose tq [ns, cols] lists, per support, the queries
// that read it -- the edges (q, j) with idx[q, j] = s in ascending (q, j) order, pads (the value nq) behind them.  With it
//   dx[s] = sum over the edges into s of (what the scatter kernels add to row s for that edge)
// is a sum one wavefront owns: no atomics, a fixed order, the same bits run after run in either arithmetic mode.  For KPConv
// the sum IS a KPConv on the transposed graph (queries and supports swap, the kernel points change sign), so it runs on the
// forward's gather kernels (kpconv.hip) and one product.
//
// The transposition: count (integer atomics on deg), exclusive scan, scatter of the keys q * h + j into a raw CSR segment
// per support through an atomic cursor (arrival order), then one wavefront per support RANKS its segment: an edge goes to
// position = the number of smaller keys of its segment.  Keys are unique, so the ranks are a permutation of 0 .. deg - 1 and
// the table does not depend on scheduling; the placement is out of place (raw -> tq), so there is no hazard between readers
// and writers.  deg / 64 segment loads and deg readlane-compares per edge.
#include "pcrcg_train.h"
#include "kpconv.h"
#include "trainops.h"

namespace pcrcg {
namespace {

constexpr int K = PCRCG_KPOINTS;

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const int o = __shfl_xor(v, d, 64); v = o > v ? o : v; }
    return v;
}

// one lane per table entry: deg[idx] += 1 for the real ones
__global__ void __launch_bounds__(256) k_tr_count(const long long* __restrict__ idx, long total, int h, int ld_idx, int ns,
                                                   int* __restrict__ deg) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const long q = t / h;
    const long long v = idx[q * ld_idx + (t - q * h)];
    if (v >= 0 && v < ns) atomicAdd(&deg[v], 1);
}
// stats = (sum, max) of deg: a few workgroups stride over it and every wavefront adds ONCE -- tens of thousands of
// wavefronts adding to one address (the count kernel's own lanes, first version) cost 0.4 ms at 2.6 M entries
constexpr int kStatBlocks = 64;
__global__ void __launch_bounds__(256) k_tr_degstats(const int* __restrict__ deg, int ns, int* __restrict__ stats) {
    int sum = 0, mx = 0;
    for (int s = blockIdx.x * 256 + threadIdx.x; s < ns; s += gridDim.x * 256) {
        const int d = deg[s];
        sum += d;
        mx = d > mx ? d : mx;
    }
    sum = wave_sum(sum);
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0 && mx) {
        atomicAdd(&stats[0], sum);
        atomicMax(&stats[1], mx);
    }
}

// one lane per table entry: its key into the raw segment of its support, at the position an atomic cursor hands out.
// A `deg` that does not belong to this table (the caller's mistake) must not become a store outside raw [cap]: an edge the
// segment has no room for is dropped.
__global__ void __launch_bounds__(256) k_tr_scatter(const long long* __restrict__ idx, long total, int h, int ld_idx, int ns,
                                                     const int* __restrict__ deg, const int* __restrict__ start,
                                                     int* __restrict__ cursor, int* __restrict__ raw, long cap) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const long q = t / h;
    const long long v = idx[q * ld_idx + (t - q * h)];
    if (v < 0 || v >= ns) return;
    const int at = atomicAdd(&cursor[v], 1);
    const long p = (long)start[v] + at;
    if (at < deg[v] && p >= 0 && p < cap) raw[p] = (int)t;             // t = q * h + j < 2^31 (checked on the host)
}

// One wavefront per support row: the keys of its raw segment sit in lanes, 64 at a time; a key's rank = the number of
// smaller keys of the segment (keys are unique), counted against the segment passed round by v_readlane; the edge lands at
// that rank as (query, column) = (key / h, key % h) -- neighbouring ranks from neighbouring lanes' stores -- and the pads
// behind the row's edges follow.  status = 1 when the row holds more edges than columns (every writer stores the same 1).
__global__ void __launch_bounds__(256) k_tr_place_rows(const int* __restrict__ deg, const int* __restrict__ start,
                                                        const int* __restrict__ raw, long cap, int ns, int h, int cols,
                                                        long long nq, long long* __restrict__ tq, int ld_tq,
                                                        int* __restrict__ th, int ld_th, int* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const long s = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (s >= ns) return;
    const int d = deg[s];
    const long p0 = start[s];
    int n = d > 0 ? d : 0;                                            // a segment must lie inside raw [cap], whatever deg says
    if (p0 < 0 || p0 > cap) n = 0;
    else if (p0 + n > cap) n = (int)(cap - p0);
    for (int a0 = 0; a0 < n; a0 += 64) {
        const int a = a0 + lane;
        const int key = a < n ? raw[p0 + a] : 0x7fffffff;
        int rank = 0;
        for (int b0 = 0; b0 < n; b0 += 64) {
            const int b = b0 + lane;
            const int other = b < n ? raw[p0 + b] : 0x7fffffff;
            const int nb = n - b0 < 64 ? n - b0 : 64;
            for (int e = 0; e < nb; ++e) rank += __shfl(other, e, 64) < key ? 1 : 0;
        }
        if (a < n && rank < cols) {
            tq[s * ld_tq + rank] = key / h;
            if (th) th[s * ld_th + rank] = key % h;
        }
    }
    for (int c = n + lane; c < cols; c += 64) {
        tq[s * ld_tq + c] = nq;
        if (th) th[s * ld_th + c] = -1;
    }
    if (lane == 0 && d > cols) *status = 1;
}

__global__ void __launch_bounds__(64) k_negate(const float* __restrict__ src, float* __restrict__ dst, int n) {
    const int t = threadIdx.x;
    if (t < n) dst[t] = -src[t];
}

// ---- max_pool backward as a gather -----------------------------------------------------------------------------------
// One wavefront per (support row s, 64-channel chunk), lanes = channels.  For every edge (q, j) into s, in table order: the
// row receives dy[q, c] iff x[s, c] attains y[q, c] and no EARLIER column of row q does -- the walk of k_gather_max_bwd
// (trainops.hip) cut at column j: a shadow counts as the value 0 and swallows the gradient when it comes first, an earlier
// real column of the same value wins.  The walk is wave-uniform in its bounds (q and j are) and ends as soon as every
// candidate channel has met an earlier maximum.
__global__ void __launch_bounds__(256) k_gather_max_bwd_t(const float* __restrict__ x, int ns, int c,
                                                           const long long* __restrict__ idx, int nq, int h, int ld_idx,
                                                           const float* __restrict__ y, const float* __restrict__ dy,
                                                           const long long* __restrict__ tq, const int* __restrict__ th,
                                                           int cols, int ld_t, float* __restrict__ dx, int nchunk) {
    const int lane = threadIdx.x & 63;
    const long item = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (item >= (long)ns * nchunk) return;
    const int s = (int)(item / nchunk), chunk = (int)(item - (long)s * nchunk);
    const int cc = chunk * 64 + lane;
    const bool cok = cc < c;
    const int cl = cok ? cc : c - 1;                                  // clamped: loads stay inside the row
    const float xv = x[(long)s * c + cl];
    float acc = 0.f;
    for (int e = 0; e < cols; ++e) {
        const long long qv = tq[(long)s * ld_t + e];
        if (qv < 0 || qv >= nq) break;                                // pads trail
        const int q = (int)qv;
        int j = th[(long)s * ld_t + e];
        j = j < 0 ? 0 : (j < h ? j : h - 1);                          // a column outside the table must not become an address
        const float m = y[(long)q * c + cl];
        bool open = cok && xv == m;
        const long long* row = idx + (long)q * ld_idx;
        for (int jn = 0; jn < j && __ballot(open); ++jn) {
            const long long i = row[jn];
            const bool real = i >= 0 && i < ns;
            const float v = real ? x[i * c + cl] : 0.f;
            if (v == m) open = false;
        }
        if (open) acc += dy[(long)q * c + cl];
    }
    if (cok) dx[(long)s * c + cc] = acc;
}

// closest_pool backward as a gather: dx[s, :] = sum over the edges into s of dy[q, :], in table order
__global__ void __launch_bounds__(256) k_gather_first_bwd_t(const float* __restrict__ dy, int ld_dy, int c,
                                                             const long long* __restrict__ tq, int cols, int ld_tq, int nq,
                                                             int ns, float* __restrict__ dx, int ld_dx, int nchunk) {
    const int lane = threadIdx.x & 63;
    const long item = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (item >= (long)ns * nchunk) return;
    const int s = (int)(item / nchunk), chunk = (int)(item - (long)s * nchunk);
    const int cc = chunk * 64 + lane;
    if (cc >= c) return;
    float acc = 0.f;
    for (int e = 0; e < cols; ++e) {
        const long long qv = tq[(long)s * ld_tq + e];
        if (qv < 0 || qv >= nq) break;                                // pads trail
        acc += dy[qv * ld_dy + cc];
    }
    dx[(long)s * ld_dx + cc] = acc;
}

inline size_t count1(long n) { return (size_t)(n > 0 ? n : 1); }

}  // namespace
}  // namespace pcrcg

using namespace pcrcg;

extern "C" int pcrcg_neighbors_transpose_count(const int64_t* idx, int nq, int h, int ld_idx, int ns, int* deg, int* stats,
                                               void* stream) {
    PCRCG_CHECK_ARG(nq >= 0 && ns >= 0 && h >= 1 && ld_idx >= h);
    PCRCG_CHECK_ARG((long)nq * h < (1L << 31));
    PCRCG_CHECK_ARG(stats && (deg || ns == 0) && (idx || nq == 0));
    hipStream_t st = as_stream(stream);
    PCRCG_CHECK_HIP(hipMemsetAsync(stats, 0, 2 * sizeof(int), st));
    if (ns == 0) return PCRCG_OK;
    PCRCG_CHECK_HIP(hipMemsetAsync(deg, 0, (size_t)ns * sizeof(int), st));
    const long total = (long)nq * h;
    if (total == 0) return PCRCG_OK;
    hipLaunchKernelGGL(k_tr_count, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                       reinterpret_cast<const long long*>(idx), total, h, ld_idx, ns, deg);
    const int sb = (ns + 255) / 256 < kStatBlocks ? (ns + 255) / 256 : kStatBlocks;
    hipLaunchKernelGGL(k_tr_degstats, dim3(sb), dim3(256), 0, st, deg, ns, stats);
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}

// ws: [ row starts [ns] | cursors [ns] | raw keys [nq * h] | scan scratch ]
extern "C" size_t pcrcg_neighbors_transpose_ws_bytes(int nq, int h, int ns) {
    if (nq < 0 || h < 1 || ns < 0 || (long)nq * h >= (1L << 31)) return 0;
    return 2 * carve_bytes(count1(ns), sizeof(int)) + carve_bytes(count1((long)nq * h), sizeof(int)) + scan_ws_bytes(ns);
}

extern "C" int pcrcg_neighbors_transpose_fill(const int64_t* idx, int nq, int h, int ld_idx, int ns, const int* deg, int cols,
                                              int64_t* tq, int ld_tq, int* th, int ld_th, int* status, void* ws,
                                              size_t ws_bytes, void* stream) {
    PCRCG_CHECK_ARG(nq >= 0 && ns >= 0 && h >= 1 && ld_idx >= h);
    PCRCG_CHECK_ARG((long)nq * h < (1L << 31));
    PCRCG_CHECK_ARG(cols >= 1 && ld_tq >= cols && (!th || ld_th >= cols));
    PCRCG_CHECK_ARG(status && ((deg && tq && ws) || ns == 0) && (idx || nq == 0));
    hipStream_t st = as_stream(stream);
    PCRCG_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int), st));
    if (ns == 0) return PCRCG_OK;
    const long total = (long)nq * h;
    Carver cv(ws, ws_bytes);
    int* start = cv.take<int>(count1(ns));
    int* cursor = cv.take<int>(count1(ns));
    int* raw = cv.take<int>(count1(total));
    void* scan_ws = cv.take<char>(scan_ws_bytes(ns));
    PCRCG_CHECK_WS(cv);
    PCRCG_PROPAGATE(exclusive_scan_i32(deg, start, ns, nullptr, scan_ws, st));
    if (total > 0) {
        PCRCG_CHECK_HIP(hipMemsetAsync(cursor, 0, (size_t)ns * sizeof(int), st));
        hipLaunchKernelGGL(k_tr_scatter, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                           reinterpret_cast<const long long*>(idx), total, h, ld_idx, ns, deg, start, cursor, raw, total);
    }
    hipLaunchKernelGGL(k_tr_place_rows, dim3((ns + 3) / 4), dim3(256), 0, st, deg, start, raw, total, ns, h, cols, (long long)nq,
                       reinterpret_cast<long long*>(tq), ld_tq, th, ld_th, status);
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}

// ws: [ g = dy * inv_n [nq, cout] | -kp [15, 3] | wf' [ns, 15 * cout] | the aggregate's 1 / n [ns] (unused) | its scratch ]
extern "C" size_t pcrcg_kpconv_backward_dx_t_ws_bytes(int nq, int ns, int cout) {
    if (nq < 0 || ns < 0 || cout < 1) return 0;
    return carve_bytes(count1(nq) * (size_t)cout, 4) + carve_bytes(3 * K, 4) + carve_bytes(count1(ns) * K * (size_t)cout, 4) +
           carve_bytes(count1(ns), 4) + pcrcg_kpconv_ws_bytes(nq);
}

extern "C" int pcrcg_kpconv_backward_dx_t(const float* q_pts, int nq, const float* s_pts, int ns, const int64_t* tq, int cols,
                                          int ld_tq, const float* dy, int ld_dy, const float* inv_n, int cout, const float* kp,
                                          float extent, const float* wt, int cin, float* dx, int ld_dx, void* ws,
                                          size_t ws_bytes, void* stream) {
    PCRCG_CHECK_ARG(nq >= 0 && ns >= 0 && cols >= 1 && ld_tq >= cols && cout >= 1 && cin >= 1 && ld_dy >= cout && ld_dx >= cin);
    PCRCG_CHECK_ARG(extent > 0.0f);
    if (ns == 0) return PCRCG_OK;
    PCRCG_CHECK_ARG(dx && s_pts && tq && kp && wt && ws && ((q_pts && dy && inv_n) || nq == 0));
    hipStream_t st = as_stream(stream);
    if (nq == 0) {                                                   // no edge: every row of dx is zero
        PCRCG_CHECK_HIP(hipMemset2DAsync(dx, (size_t)ld_dx * 4, 0, (size_t)cin * 4, (size_t)ns, st));
        return PCRCG_OK;
    }
    Carver cv(ws, ws_bytes);
    float* g = cv.take<float>((size_t)nq * cout);
    float* kpn = cv.take<float>(3 * K);
    float* wf = cv.take<float>((size_t)ns * K * cout);
    float* inv = cv.take<float>((size_t)ns);
    const size_t agg_bytes = pcrcg_kpconv_ws_bytes(nq);
    void* agg = cv.take<char>(agg_bytes);
    PCRCG_CHECK_WS(cv);
    PCRCG_PROPAGATE(tr_scale_rows(dy, ld_dy, inv_n, g, nq, cout, st));
    hipLaunchKernelGGL(k_negate, dim3(1), dim3(64), 0, st, kp, kpn, 3 * K);
    PCRCG_CHECK_LAUNCH();
    // the supports are the queries of the transposed problem, g its features, nq its shadow index
    KpconvCall gather;
    gather.q_pts = s_pts; gather.nq = ns; gather.s_pts = q_pts; gather.ns = nq;
    gather.idx = tq; gather.h = cols; gather.ld_idx = ld_tq;
    gather.x = g; gather.cin = cout; gather.kp = kpn; gather.extent = extent;
    gather.wf = wf; gather.inv_n = inv; gather.ws = agg; gather.ws_bytes = agg_bytes; gather.st = st;
    PCRCG_PROPAGATE(kpconv_run(gather));
    return pcrcg_gemm_f32_grad(wf, K * cout, 0, wt, cin, 0, dx, ld_dx, ns, cin, K * cout, nullptr, nullptr, 1, stream);
}

extern "C" int pcrcg_gather_max_backward_t(const float* x, int ns, int c, const int64_t* idx, int nq, int h, int ld_idx,
                                           const float* y, const float* dy, const int64_t* tq, const int* th, int cols, int ld_t,
                                           float* dx, void* stream) {
    PCRCG_CHECK_ARG(ns >= 0 && c >= 1 && nq >= 0 && h >= 1 && ld_idx >= h && cols >= 1 && ld_t >= cols);
    if (ns == 0) return PCRCG_OK;
    PCRCG_CHECK_ARG(x && tq && th && dx && ((idx && y && dy) || nq == 0));
    const int nchunk = (c + 63) / 64;
    const long items = (long)ns * nchunk;
    hipLaunchKernelGGL(k_gather_max_bwd_t, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, as_stream(stream), x, ns, c,
                       reinterpret_cast<const long long*>(idx), nq, h, ld_idx, y, dy, reinterpret_cast<const long long*>(tq), th,
                       cols, ld_t, dx, nchunk);
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}

extern "C" int pcrcg_gather_first_backward_t(const float* dy, int ld_dy, int c, const int64_t* tq, int cols, int ld_tq, int nq,
                                             int ns, float* dx, int ld_dx, void* stream) {
    PCRCG_CHECK_ARG(c >= 1 && nq >= 0 && ns >= 0 && cols >= 1 && ld_tq >= cols && ld_dy >= c && ld_dx >= c);
    if (ns == 0) return PCRCG_OK;
    PCRCG_CHECK_ARG(tq && dx && (dy || nq == 0));
    const int nchunk = (c + 63) / 64;
    const long items = (long)ns * nchunk;
    hipLaunchKernelGGL(k_gather_first_bwd_t, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, as_stream(stream), dy, ld_dy, c,
                       reinterpret_cast<const long long*>(tq), cols, ld_tq, nq, ns, dx, ld_dx, nchunk);
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}
