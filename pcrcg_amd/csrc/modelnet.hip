// modelnet.hip -- ModelNet pair preparation (ref:datasets/transforms.py RandomCrop, RandomTransformSE3_euler, Resampler,
// RandomJitter, ShufflePoints after their random numbers are drawn; include/pcrcg.h "ModelNet pair preparation" has the
// arithmetic contract, DESIGN.md section 16 the reasons).
//
// k_modelnet_crop: one workgroup of 1024 threads per cloud, the cloud's float64 plane distances resident in LDS.
//   1. rows staged through LDS 1024 at a time; three lanes add the columns in float32 in row order (numpy's mean over axis 0
//      adds rows one after another, so a tree would round differently); any non-finite coordinate rejects the cloud;
//   2. dist[i] = (f64(cx) d0 + f64(cy) d1) + f64(cz) d2 of the float32 differences c = p - centroid, unfused;
//   3. percentile mode: a bitonic sort of a copy of dist (padded with +inf to a power of two) gives the two order statistics,
//      the threshold is numpy's lerp of them;
//   4. a stable compaction of the rows with dist > threshold, 1024 rows per block scan.
// k_modelnet_assemble: one output row per thread, out[i] = f32(f64(T . raw[kept[pick[i]]]) + noise[i]).
// Plain stores, no atomics on memory, no workspace.
#include "block_scan.h"
#include "common.h"

namespace pcrcg {
namespace {

constexpr int kCropThreads = 1024;
constexpr int kCropMaxRows = PCRCG_MODELNET_CROP_MAX_ROWS;

struct CropArgs {
    const float* pts; const int* off; const int* mode; const double* dir; const int* lo; const double* gamma;
    int* kept; int* count;
    int ld, n_total, max_rows;
};

__global__ void __launch_bounds__(kCropThreads) k_modelnet_crop(CropArgs a) {
    extern __shared__ double lds[];                  // dist [max_rows] | sorted copy [pow2 >= max_rows]
    __shared__ float stage[kCropThreads * 3];
    __shared__ float cen[3];
    __shared__ int scan_sm[kCropThreads / 64];
    __shared__ int bad;
    const int c = blockIdx.x, tid = threadIdx.x;
    const int begin = a.off[c], end = a.off[c + 1];
    // (every exit below is taken by the whole workgroup: its condition depends on the cloud alone)
    if (begin < 0 || end < begin || end > a.n_total) {
        if (tid == 0) a.count[c] = 0;
        return;
    }
    const int n = end - begin, mode = a.mode[c];
    if (n > a.max_rows || mode < 0 || mode > 2) {
        if (tid == 0) a.count[c] = -1;
        return;
    }
    if (n == 0) {
        if (tid == 0) a.count[c] = 0;
        return;
    }
    const float* p = a.pts + (size_t)begin * a.ld;
    int* kept = a.kept + begin;
    double* dist = lds;
    double* srt = lds + a.max_rows;

    if (tid == 0) bad = 0;
    __syncthreads();
    float acc = 0.0f;
    for (int base = 0; base < n; base += kCropThreads) {
        const int i = base + tid;
        if (i < n) {
            const float x = p[(size_t)i * a.ld], y = p[(size_t)i * a.ld + 1], z = p[(size_t)i * a.ld + 2];
            stage[tid * 3] = x; stage[tid * 3 + 1] = y; stage[tid * 3 + 2] = z;
            if (!(isfinite(x) && isfinite(y) && isfinite(z))) bad = 1;
        }
        __syncthreads();
        if (tid < 3) {
            const int rows = n - base < kCropThreads ? n - base : kCropThreads;
            for (int r = 0; r < rows; ++r) acc += stage[r * 3 + tid];
        }
        __syncthreads();
    }
    if (bad) {
        if (tid == 0) a.count[c] = -1;
        return;
    }
    if (mode == 0) {
        for (int i = tid; i < n; i += kCropThreads) kept[i] = i;
        if (tid == 0) a.count[c] = n;
        return;
    }
    if (tid < 3) cen[tid] = acc / (float)n;
    __syncthreads();

    const double d0 = a.dir[(size_t)c * 3], d1 = a.dir[(size_t)c * 3 + 1], d2 = a.dir[(size_t)c * 3 + 2];
    int P = 1;
    while (P < n) P <<= 1;
    for (int i = tid; i < n; i += kCropThreads) {
        const float cx = p[(size_t)i * a.ld] - cen[0], cy = p[(size_t)i * a.ld + 1] - cen[1], cz = p[(size_t)i * a.ld + 2] - cen[2];
        const double d = ((double)cx * d0 + (double)cy * d1) + (double)cz * d2;
        dist[i] = d;
        if (mode == 2) srt[i] = d;
    }
    double thr = 0.0;
    if (mode == 2) {
        for (int i = n + tid; i < P; i += kCropThreads) srt[i] = INFINITY;
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < (P >> 1); t += kCropThreads) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                    const bool up = (i & k) == 0;
                    const double x = srt[i], y = srt[l];
                    if ((x > y) == up) { srt[i] = y; srt[l] = x; }
                }
                __syncthreads();
            }
        }
        int lo = a.lo[c];
        lo = lo < 0 ? 0 : (lo > n - 1 ? n - 1 : lo);
        const double g = a.gamma[c];
        const double va = srt[lo];
        if (lo + 1 == n) {
            thr = va;
        } else {
            const double vb = srt[lo + 1], diff = vb - va;
            thr = g >= 0.5 ? vb - diff * (1.0 - g) : va + diff * g;
        }
    } else {
        __syncthreads();
    }

    int run = 0;
    for (int base = 0; base < n; base += kCropThreads) {
        const int i = base + tid;
        const int f = (i < n && dist[i] > thr) ? 1 : 0;
        int tot;
        const int e = block_excl_scan_i32<kCropThreads>(f, &tot, scan_sm);
        if (f) kept[run + e] = i;
        run += tot;
    }
    if (tid == 0) a.count[c] = run;
}

struct AssembleArgs {
    const float* raw; const int* in_off; const int* kept; const int* kept_count;
    const int* out_off; const int* out_cloud; const int* out_flags; const float* tf; const int* pick; const double* noise;
    float* out;
    int ld, n_total, C, K, m_total;
};

__global__ void __launch_bounds__(256) k_modelnet_assemble(AssembleArgs a) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.m_total) return;
    int lo = 0, hi = a.K - 1;                        // the last output cloud that starts at or before row i
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.out_off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    const int k = lo;
    if (!(a.out_off[k] <= i && i < a.out_off[k + 1])) return;
    float* o = a.out + (size_t)i * a.ld;
    const int c = a.out_cloud[k];
    long row = -1;
    if (c >= 0 && c < a.C) {
        const int begin = a.in_off[c], end = a.in_off[c + 1];
        if (begin >= 0 && end >= begin && end <= a.n_total) {
            const int n = end - begin, cnt = a.kept ? a.kept_count[c] : n, pk = a.pick[i];
            if (cnt <= n && pk >= 0 && pk < cnt) {
                const int r = a.kept ? a.kept[begin + pk] : pk;
                if (r >= 0 && r < n) row = (long)begin + r;
            }
        }
    }
    if (row < 0) {                                   // an index that points nowhere: the row says so
        for (int q = 0; q < a.ld; ++q) o[q] = NAN;
        return;
    }
    const float* s = a.raw + (size_t)row * a.ld;
    const int flags = a.out_flags[k];
    float x = s[0], y = s[1], z = s[2];
    const bool moved = (flags & 1) && a.tf, noisy = (flags & 2) && a.noise;      // (a flag without its array does nothing)
    const float* T = moved ? a.tf + (size_t)k * 12 : nullptr;
    if (moved) {
        const float X = ((x * T[0] + y * T[1]) + z * T[2]) + T[3];
        const float Y = ((x * T[4] + y * T[5]) + z * T[6]) + T[7];
        const float Z = ((x * T[8] + y * T[9]) + z * T[10]) + T[11];
        x = X; y = Y; z = Z;
    }
    if (noisy) {
        const double* nz = a.noise + (size_t)i * 3;
        x = (float)((double)x + nz[0]);
        y = (float)((double)y + nz[1]);
        z = (float)((double)z + nz[2]);
    }
    o[0] = x; o[1] = y; o[2] = z;
    if (a.ld == 6) {
        float u = s[3], v = s[4], w = s[5];
        if (moved) {
            const float U = (u * T[0] + v * T[1]) + w * T[2];
            const float V = (u * T[4] + v * T[5]) + w * T[6];
            const float W = (u * T[8] + v * T[9]) + w * T[10];
            u = U; v = V; w = W;
        }
        o[3] = u; o[4] = v; o[5] = w;
    }
}

}  // namespace
}  // namespace pcrcg

using namespace pcrcg;

extern "C" {

int pcrcg_modelnet_crop(const float* pts, int ld, int n_total, const int* off, int C, int max_rows, const int* mode,
                        const double* dir, const int* lo, const double* gamma, int* kept, int* count, void* stream) {
    PCRCG_CHECK_ARG(pts && off && mode && dir && lo && gamma && kept && count);
    PCRCG_CHECK_ARG(ld == 3 || ld == 6);
    PCRCG_CHECK_ARG(n_total >= 0 && n_total <= (1 << 30) && C >= 1 && C <= (1 << 20));
    PCRCG_CHECK_ARG(max_rows >= 1);
    if (max_rows > kCropMaxRows) {
        set_error("pcrcg_modelnet_crop: a cloud of %d rows is longer than a workgroup holds (%d)", max_rows, kCropMaxRows);
        return PCRCG_EBADARG;
    }
    int P = 1;
    while (P < max_rows) P <<= 1;
    const size_t dyn = (size_t)(max_rows + P) * sizeof(double);
    PCRCG_GRANT_LDS(k_modelnet_crop);
    CropArgs a;
    a.pts = pts; a.off = off; a.mode = mode; a.dir = dir; a.lo = lo; a.gamma = gamma; a.kept = kept; a.count = count;
    a.ld = ld; a.n_total = n_total; a.max_rows = max_rows;
    hipLaunchKernelGGL(k_modelnet_crop, dim3((unsigned)C), dim3(kCropThreads), dyn, as_stream(stream), a);
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}

int pcrcg_modelnet_assemble(const float* raw, int ld, int n_total, const int* in_off, int C, const int* kept,
                            const int* kept_count, const int* out_off, const int* out_cloud, const int* out_flags,
                            const float* tf, int K, const int* pick, const double* noise, int m_total, float* out,
                            void* stream) {
    PCRCG_CHECK_ARG(raw && in_off && out_off && out_cloud && out_flags && pick && out);
    PCRCG_CHECK_ARG((kept == nullptr) == (kept_count == nullptr));
    PCRCG_CHECK_ARG(ld == 3 || ld == 6);
    PCRCG_CHECK_ARG(n_total >= 0 && n_total <= (1 << 30) && C >= 1 && C <= (1 << 20) && K >= 1 && K <= (1 << 20));
    PCRCG_CHECK_ARG(m_total >= 0 && m_total <= (1 << 30));
    if (m_total == 0) return PCRCG_OK;
    AssembleArgs a;
    a.raw = raw; a.in_off = in_off; a.kept = kept; a.kept_count = kept_count; a.out_off = out_off; a.out_cloud = out_cloud;
    a.out_flags = out_flags; a.tf = tf; a.pick = pick; a.noise = noise; a.out = out;
    a.ld = ld; a.n_total = n_total; a.C = C; a.K = K; a.m_total = m_total;
    hipLaunchKernelGGL(k_modelnet_assemble, dim3((unsigned)((m_total + 255) / 256)), dim3(256), 0, as_stream(stream), a);
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}

}
