// voxel.hip -- batched open3d-style voxel down-sampling of raw scans on gfx950: what ref:datasets/kitti.py:134-140 does to
// both scans of a pair with pcd.voxel_down_sample(first_subsampling_dl).  ABI: include/pcrcg.h, section "Voxel
// down-sampling"; DESIGN.md section 14 defines the operation, tests/voxel_ref.py restates it in numpy.
//
// This is NOT grid_subsample.hip's operation: open3d's grid starts at min - voxel / 2 (there: floor(min / dl) * dl) and
// every step is float64 (there: fp32).  What the two share is the machinery -- a per-cloud open-addressing hash table,
// first-occurrence ranks from a device scan, per-cell id lists -- restated here for float64 rows and DEVICE offsets.
// Pipeline (all on the caller's stream, no host round trip):
//
//   1 init     : the offsets become disjoint ascending ranges (anything else reads as an empty cloud); tables reset
//   2 min/max  : per cloud and axis, ordered-uint atomics on the fp32 coordinates (wave pre-reduced); a non-finite
//                coordinate marks its cloud rejected
//   3 insert   : per point, in float64: idx = (int)floor((p - (min - voxel / 2)) / voxel), 21 bits per axis packed into one
//                key -> the cloud's hash table (one 64-bit CAS), atomicMin of the first input index, atomicAdd of the count.
//                A cloud whose largest index would reach 2^21 is rejected (every thread of it sees that from the maximum).
//   4 rank     : flag first occurrences, device scan -> output row of every voxel = the order of first input points.
//                Clouds are contiguous in the input, so cloud b's rows follow cloud b-1's with no gap.
//   5 lists    : scan of the counts -> per-voxel segments; scatter the point ids (atomic cursor: any order)
//   6 average  : one thread per voxel sorts its ids ascending and adds the points ONE BY ONE in input order in float64,
//                then divides by (double)count.  No floating-point atomics: a cloud's bits depend on its points and the
//                voxel size alone.  A cloud that falls into one voxel is one thread's work: slow but correct.
//   7 lengths  : out_len[b] = rows of cloud b, or -1 for a rejected cloud
//
// Compiled with -ffp-contract=off (every operation rounds where the source says).
#include "block_scan.h"
#include "cellgrid.h"
#include "common.h"

namespace pcrcg {
namespace {

constexpr int kInfIdx = 0x7FFFFFFF;
constexpr int kVoxelMaxBatch = 65535;
constexpr int kVoxelMaxRows = 1 << 30;          // table slots (2 per row) are addressed with 32-bit integers
constexpr double kVoxelIndexLimit = 2097152.0;  // 2^21: three indices share one 64-bit key
constexpr int kVoxelMinmaxBlocks = 64;
constexpr int kNonFinite = 1;                   // status bit

__device__ __forceinline__ unsigned enc_f32(float f) {      // fp32 -> unsigned with the same order
    unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float dec_f32(unsigned u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}

struct VoxelWs {
    int* cs;          // [B]      first row of cloud b ...
    int* ce;          // [B]      ... and one past its last: disjoint, ascending
    unsigned* mm;     // [B, 6]   ordered-uint min[3] | max[3]
    int* status;      // [B]
    u64* tkey;        // [2 N]    cloud b's table: slots 2 cs[b] .. 2 ce[b]
    int* tfirst;      // [2 N]    lowest input row of the slot's voxel
    int* tcnt;        // [2 N]
    int* trank;       // [2 N]    its output row
    int* slot_of;     // [N]      -1: the row belongs to no cloud or to a rejected one
    int* rank;        // [N + 1]  flags, then their exclusive scan; rank[n_total] = all rows written
    int* ccnt;        // [N]      per output row: points ...
    int* cstart;      // [N]      ... and where its id list starts
    int* cfill;       // [N]
    int* cidx;        // [N]
    void* scan_ws;
};

VoxelWs carve_voxel(Carver& cv, int B, int n_total) {
    const size_t N = (size_t)n_total + 1;
    VoxelWs w;
    w.cs = cv.take<int>((size_t)B);
    w.ce = cv.take<int>((size_t)B);
    w.mm = cv.take<unsigned>((size_t)B * 6);
    w.status = cv.take<int>((size_t)B);
    w.tkey = cv.take<u64>(2 * N);
    w.tfirst = cv.take<int>(2 * N);
    w.tcnt = cv.take<int>(2 * N);
    w.trank = cv.take<int>(2 * N);
    w.slot_of = cv.take<int>(N);
    w.rank = cv.take<int>(N + 1);
    w.ccnt = cv.take<int>(N);
    w.cstart = cv.take<int>(N);
    w.cfill = cv.take<int>(N);
    w.cidx = cv.take<int>(N);
    w.scan_ws = cv.take<char>(scan_ws_bytes(n_total + 1));
    return w;
}

// the cloud that holds row i, or -1 (ranges are disjoint and ascending; an empty cloud starts where it ends)
__device__ __forceinline__ int cloud_of(const int* __restrict__ cs, const int* __restrict__ ce, int B, int i) {
    int lo = 0, hi = B - 1;   // largest b with cs[b] <= i
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (cs[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return (cs[lo] <= i && i < ce[lo]) ? lo : -1;
}

// vmin = min - voxel / 2 per axis; false: the cloud is rejected (a non-finite coordinate, or an index that would reach 2^21
// -- (p - vmin) / voxel is monotonic in p, so the cloud's maximum decides for all its points)
__device__ __forceinline__ bool cloud_frame(const unsigned* __restrict__ mm, const int* __restrict__ status, int b, double voxel,
                                            double* vmin) {
    if (status[b] != 0) return false;
    bool ok = true;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        vmin[d] = (double)dec_f32(mm[6 * b + d]) - 0.5 * voxel;
        const double top = floor(((double)dec_f32(mm[6 * b + 3 + d]) - vmin[d]) / voxel);
        ok = ok && top < kVoxelIndexLimit;      // (false for a NaN too)
    }
    return ok;
}

__global__ void __launch_bounds__(256) k_voxel_init(const int* __restrict__ off, int B, int n_total, VoxelWs w) {
    const long t0 = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
    const long N = (long)n_total + 1;
    if (t0 == 0) {
        int prev_end = 0;
        for (int b = 0; b < B; ++b) {
            const int lo = off[b], hi = off[b + 1];
            const bool ok = lo >= prev_end && lo <= hi && hi <= n_total;
            w.cs[b] = ok ? lo : prev_end;
            w.ce[b] = ok ? hi : prev_end;
            if (ok) prev_end = hi;
        }
    }
    for (long i = t0; i < (long)B * 6; i += stride) w.mm[i] = (i % 6) < 3 ? 0xFFFFFFFFu : 0u;
    for (long i = t0; i < B; i += stride) w.status[i] = 0;
    for (long i = t0; i < 2 * N; i += stride) { w.tkey[i] = kEmptyKey; w.tfirst[i] = kInfIdx; w.tcnt[i] = 0; }
    for (long i = t0; i < N; i += stride) { w.ccnt[i] = 0; w.cfill[i] = 0; }
}

// Bounding box per cloud.  A workgroup walks a contiguous slice of the rows, so it sees at most a couple of clouds; a
// wavefront reduces what it saw of one cloud with shuffles and issues one atomic per component when the cloud changes.
__global__ void __launch_bounds__(256) k_voxel_minmax(const float* __restrict__ pts, int B, int n_total, VoxelWs w) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int per = (n_total + gridDim.x - 1) / gridDim.x;
    const long begin = (long)blockIdx.x * per;
    const int end = (int)min((long)n_total, begin + per);
    int cur = -1;
    unsigned lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
    auto flush = [&](int cloud) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            unsigned l = lo[d], h = hi[d];
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) {
                l = min(l, (unsigned)__shfl_xor((int)l, s, 64));
                h = max(h, (unsigned)__shfl_xor((int)h, s, 64));
            }
            if (lane == 0 && cloud >= 0 && h >= l) {
                atomicMin(&w.mm[cloud * 6 + d], l);
                atomicMax(&w.mm[cloud * 6 + 3 + d], h);
            }
            lo[d] = 0xFFFFFFFFu;
            hi[d] = 0u;
        }
    };
    for (long base = begin + wave * 64; base < end; base += 256) {
        const long i = base + lane;
        const bool valid = i < end;
        const int b = valid ? cloud_of(w.cs, w.ce, B, (int)i) : -1;
        float p[3] = {0.f, 0.f, 0.f};
        bool finite = true;
        if (b >= 0) {
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                p[d] = pts[3 * i + d];
                finite = finite && fabsf(p[d]) <= 3.40282346638528859812e38f;     // (false for a NaN)
            }
            if (!finite) atomicOr(&w.status[b], kNonFinite);
        }
        const int b0 = __shfl(b, 0, 64);
        const bool uniform = __all(!valid || b == b0);
        if (uniform) {
            if (b0 != cur) { flush(cur); cur = b0; }
            if (b >= 0 && finite) {
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const unsigned e = enc_f32(p[d]);
                    lo[d] = min(lo[d], e);
                    hi[d] = max(hi[d], e);
                }
            }
        } else if (b >= 0 && finite) {   // the rare wavefront that straddles two clouds: per-lane atomics
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const unsigned e = enc_f32(p[d]);
                atomicMin(&w.mm[b * 6 + d], e);
                atomicMax(&w.mm[b * 6 + 3 + d], e);
            }
        }
    }
    flush(cur);
}

__global__ void __launch_bounds__(256) k_voxel_insert(const float* __restrict__ pts, int B, int n_total, double voxel, VoxelWs w) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_total) return;
    const int b = cloud_of(w.cs, w.ce, B, i);
    double vmin[3];
    if (b < 0 || !cloud_frame(w.mm, w.status, b, voxel, vmin)) {
        w.slot_of[i] = -1;
        return;
    }
    u64 key = 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double q = floor(((double)pts[3 * (long)i + d] - vmin[d]) / voxel);   // 0 <= q < 2^21 (cloud_frame)
        key |= (u64)(unsigned)(int)q << (21 * d);
    }
    const unsigned tsize = 2u * (unsigned)(w.ce[b] - w.cs[b]);
    const long tbase = 2l * w.cs[b];
    unsigned s = __umulhi(mix32(key), tsize);
    for (;;) {       // at most len_b distinct keys in 2 len_b slots: the probe ends
        const u64 prev = atomicCAS(&w.tkey[tbase + s], kEmptyKey, key);
        if (prev == kEmptyKey || prev == key) break;
        s = s + 1 == tsize ? 0 : s + 1;
    }
    const int slot = (int)(tbase + s);
    w.slot_of[i] = slot;
    atomicMin(&w.tfirst[slot], i);
    atomicAdd(&w.tcnt[slot], 1);
}

__global__ void __launch_bounds__(256) k_voxel_flag(int n_total, VoxelWs w) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n_total) return;
    int f = 0;
    if (i < n_total) {
        const int s = w.slot_of[i];
        f = (s >= 0 && aload(&w.tfirst[s]) == i) ? 1 : 0;
    }
    w.rank[i] = f;       // (rank[n_total] = 0: the scan leaves the number of rows there)
}

// the first point of every voxel: the voxel's output row, count, first index
__global__ void __launch_bounds__(256) k_voxel_cells(int B, int n_total, VoxelWs w, int* __restrict__ out_first,
                                                      int* __restrict__ out_count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_total) return;
    const int s = w.slot_of[i];
    if (s < 0 || aload(&w.tfirst[s]) != i) return;
    const int c = w.rank[i];
    const int cnt = aload(&w.tcnt[s]);
    w.ccnt[c] = cnt;
    w.trank[s] = c;
    if (out_first) out_first[c] = i - w.cs[cloud_of(w.cs, w.ce, B, i)];
    if (out_count) out_count[c] = cnt;
}

__global__ void __launch_bounds__(256) k_voxel_fill(int n_total, VoxelWs w) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_total) return;
    const int s = w.slot_of[i];
    if (s < 0) return;
    const int c = w.trank[s];
    w.cidx[w.cstart[c] + atomicAdd(&w.cfill[c], 1)] = i;
}

__device__ inline void sift_down(int* a, int root, int n) {
    const int v = a[root];
    for (;;) {
        int child = 2 * root + 1;
        if (child >= n) break;
        if (child + 1 < n && a[child + 1] > a[child]) ++child;
        if (a[child] <= v) break;
        a[root] = a[child];
        root = child;
    }
    a[root] = v;
}

// One thread per voxel: its point ids ascending (= input order), then the ordered float64 sum and the division.
__global__ void __launch_bounds__(256) k_voxel_average(const float* __restrict__ pts, int n_total, VoxelWs w,
                                                        double* __restrict__ out_pts) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= w.rank[n_total]) return;
    int* seg = w.cidx + w.cstart[c];
    const int cnt = w.ccnt[c];
    if (cnt <= 16) {      // a handful of ids, scattered almost in order: insertion sort
        for (int a = 1; a < cnt; ++a) {
            const int v = seg[a];
            int j = a - 1;
            while (j >= 0 && seg[j] > v) { seg[j + 1] = seg[j]; --j; }
            seg[j + 1] = v;
        }
    } else {              // a crowded voxel: heapsort, in place, n log n whatever the order
        for (int r = cnt / 2 - 1; r >= 0; --r) sift_down(seg, r, cnt);
        for (int e = cnt - 1; e > 0; --e) {
            const int t = seg[0]; seg[0] = seg[e]; seg[e] = t;
            sift_down(seg, 0, e);
        }
    }
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int a = 0; a < cnt; ++a) {
        const long i = seg[a];
        sx = sx + (double)pts[3 * i];
        sy = sy + (double)pts[3 * i + 1];
        sz = sz + (double)pts[3 * i + 2];
    }
    const double k = (double)cnt;
    out_pts[3 * (long)c] = sx / k;
    out_pts[3 * (long)c + 1] = sy / k;
    out_pts[3 * (long)c + 2] = sz / k;
}

__global__ void __launch_bounds__(256) k_voxel_lengths(int B, double voxel, VoxelWs w, int* __restrict__ out_len) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int lo = w.cs[b], hi = w.ce[b];
    double vmin[3];
    if (hi == lo) out_len[b] = 0;
    else out_len[b] = cloud_frame(w.mm, w.status, b, voxel, vmin) ? w.rank[hi] - w.rank[lo] : -1;
}

bool voxel_sizes_ok(int B, int n_total) { return B >= 1 && B <= kVoxelMaxBatch && n_total >= 0 && n_total <= kVoxelMaxRows; }

}  // namespace
}  // namespace pcrcg

using namespace pcrcg;

extern "C" {

size_t pcrcg_voxel_down_sample_ws_bytes(int B, int n_total) {
    if (!voxel_sizes_ok(B, n_total)) return 0;
    Carver cv(nullptr, 0);
    carve_voxel(cv, B, n_total);
    return cv.off;
}

int pcrcg_voxel_down_sample_batch(const float* pts, const int* off, int n_total, int B, double voxel_size, double* out_pts,
                                  int* out_len, int* out_first, int* out_count, void* ws, size_t ws_bytes, void* stream) {
    PCRCG_CHECK_ARG(pts && off && out_pts && out_len && ws);
    PCRCG_CHECK_ARG(B >= 1 && B <= kVoxelMaxBatch);
    PCRCG_CHECK_ARG(n_total >= 0 && n_total <= kVoxelMaxRows);
    PCRCG_CHECK_ARG(voxel_size > 0.0 && voxel_size <= 1.79769313486231570815e308);      // (false for a NaN)
    Carver cv(ws, ws_bytes);
    VoxelWs w = carve_voxel(cv, B, n_total);
    PCRCG_CHECK_WS(cv);
    hipStream_t st = as_stream(stream);
    const size_t slots = 2 * ((size_t)n_total + 1);
    const int init_blocks = (int)((slots + 255) / 256 < 1024 ? (slots + 255) / 256 : 1024);
    hipLaunchKernelGGL(k_voxel_init, dim3(init_blocks), dim3(256), 0, st, off, B, n_total, w);
    if (n_total > 0) {
        const int blocks = (n_total + 255) / 256, blocks1 = n_total / 256 + 1;    // blocks1 covers n_total + 1 rows
        hipLaunchKernelGGL(k_voxel_minmax, dim3(blocks < kVoxelMinmaxBlocks ? blocks : kVoxelMinmaxBlocks), dim3(256), 0, st, pts, B,
                           n_total, w);
        hipLaunchKernelGGL(k_voxel_insert, dim3(blocks), dim3(256), 0, st, pts, B, n_total, voxel_size, w);
        hipLaunchKernelGGL(k_voxel_flag, dim3(blocks1), dim3(256), 0, st, n_total, w);
        PCRCG_PROPAGATE(exclusive_scan_i32(w.rank, w.rank, n_total + 1, nullptr, w.scan_ws, st));
        hipLaunchKernelGGL(k_voxel_cells, dim3(blocks), dim3(256), 0, st, B, n_total, w, out_first, out_count);
        PCRCG_PROPAGATE(exclusive_scan_i32(w.ccnt, w.cstart, n_total, nullptr, w.scan_ws, st));
        hipLaunchKernelGGL(k_voxel_fill, dim3(blocks), dim3(256), 0, st, n_total, w);
        hipLaunchKernelGGL(k_voxel_average, dim3(blocks), dim3(256), 0, st, pts, n_total, w, out_pts);
    }
    // (n_total = 0: every cloud is empty, cs = ce = 0, and no rank is read)
    hipLaunchKernelGGL(k_voxel_lengths, dim3((B + 255) / 256), dim3(256), 0, st, B, voxel_size, w, out_len);
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}

}  // extern "C"
