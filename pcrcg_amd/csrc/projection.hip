// projection.hip -- PCR-CG's RGB-D projection (ref:projection.py Projection.projection), the fused image-feature input of
// one pair from raw frames, and the SuperGlue valid maps (ref:datasets/indoor.py:284-299).
//
// Compiled with -ffp-contract=off: the projection must round exactly like the reference's two torch.mm calls on the CPU,
// which behave as a k-ordered fused chain fma(m3, 1, fma(m2, p2, fma(m1, p1, m0 * p0))) per output value; the chain is
// written out with explicit __fmul_rn / __fmaf_rn, the perspective division with __fdiv_rn.
#include "common.h"

namespace pcrcg {
namespace {

struct Mat16 { float m[16]; };
struct ProjParams { Mat16 w2c, K; float thresh; int h, w; };

// one row of torch.mm(M, [p; 1]) as the reference's CPU GEMM rounds it
__device__ __forceinline__ float mm_row(const float* r, float p0, float p1, float p2) {
    float a = __fmul_rn(r[0], p0);
    a = __fmaf_rn(r[1], p1, a);
    a = __fmaf_rn(r[2], p2, a);
    return __fmaf_rn(r[3], 1.0f, a);
}

// Projection.projection for one point: true iff the reference keeps it, with its pixel (column px, row py).
// `.long()` truncates toward zero, so a quotient in (-1, 0) is pixel 0 and is kept; NaN / +-inf / out-of-range quotients
// become INT64_MIN on x86 and are masked -- decided here in floats, never through an integer conversion of a NaN.
// Points at or behind the camera are not rejected: the depth test alone decides, as in the reference.
__device__ __forceinline__ bool project_point(const ProjParams& P, const float* __restrict__ depth, float x, float y, float z,
                                              int& px, int& py) {
    const float c0 = mm_row(P.w2c.m + 0, x, y, z), c1 = mm_row(P.w2c.m + 4, x, y, z), c2 = mm_row(P.w2c.m + 8, x, y, z);
    const float i0 = mm_row(P.K.m + 0, c0, c1, c2), i1 = mm_row(P.K.m + 4, c0, c1, c2), i2 = mm_row(P.K.m + 8, c0, c1, c2);
    const float qx = __fdiv_rn(i0, i2), qy = __fdiv_rn(i1, i2);
    if (!(qx > -1.0f && qx < (float)P.w && qy > -1.0f && qy < (float)P.h)) return false;
    px = (int)qx;
    py = (int)qy;
    if (px >= P.w || py >= P.h) return false;          // (only reachable where (float)w rounds up: w > 2^24)
    const float d = depth[(long)py * P.w + px];
    return fabsf(__fsub_rn(i2, d)) < P.thresh;
}

// pass 1: flags[i] = kept, pix[i] = py * w + px (or -1)
__global__ void __launch_bounds__(256) k_project_flags(const float* __restrict__ pts, int n, const float* __restrict__ depth,
                                                        ProjParams P, int* __restrict__ flags, int* __restrict__ pix) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int px = 0, py = 0;
    const bool keep = project_point(P, depth, pts[3 * (long)i], pts[3 * (long)i + 1], pts[3 * (long)i + 2], px, py);
    flags[i] = keep ? 1 : 0;
    pix[i] = keep ? py * P.w + px : -1;
}

// pass 2 (after the exclusive scan of the flags into offs): stable compaction, inds3d ascending
__global__ void __launch_bounds__(256) k_project_scatter(const int* __restrict__ pix, const int* __restrict__ offs, int n, int w,
                                                          long long* __restrict__ inds2d, long long* __restrict__ inds3d) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int p = pix[i];
    if (p < 0) return;
    const int o = offs[i];
    inds2d[2 * (long)o] = p % w;
    inds2d[2 * (long)o + 1] = p / w;
    inds3d[o] = i;
}

constexpr int kMaxFrames = 6;      // up to 3 per side
struct FrameArgs { const float* fmap; const float* depth; const float* valid; ProjParams P; int target; };
struct Frames { FrameArgs f[kMaxFrames]; int n; };

// points per wavefront (8 / 16 / 32 / 64 measured at 100 / 108 / 108 / 108 us for the 4-frame S30k
// input; the gather of single floats from four 9.8 MB maps bounds the kernel, not the number of waves)
constexpr int kFramesPW = 8;

// The whole [n_points, ldx] input of one pair from raw frames: one wavefront per kFramesPW points.
//   phase 1: lane l < kFramesPW projects point base + l against the frames of its side, last frame first; the first that
//            accepts it is the reference's last writer (frames come in its write order) -- frame index and pixel stay in
//            registers
//   phase 2: the wavefront writes the rows one after another, lanes over the columns: a strided gather of c channels from
//            the winning frame's fmap [c, h, w] times its valid map [w, h] (or ones: no frame accepts the point), column c
//            = 1, columns c+1 .. ldx-1 = 0.  Every row is written exactly once.
// Frame fields are only ever indexed with compile-time constants (unrolled loops with selects): a runtime index into the
// by-value argument would put the whole array in scratch.
__global__ void __launch_bounds__(256) k_inject_frames(const float* __restrict__ pts, long n_points, long len_src, Frames fr,
                                                        int c, float* __restrict__ x, int ldx) {
    const int lane = threadIdx.x & 63;
    const long base = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * kFramesPW;
    if (base >= n_points) return;
    const long i = base + lane;
    int hit = -1, pix = 0;
    if (lane < kFramesPW && i < n_points) {
        const float px3 = pts[3 * i], py3 = pts[3 * i + 1], pz3 = pts[3 * i + 2];
        const int side = i >= len_src ? 1 : 0;
#pragma unroll
        for (int f = kMaxFrames - 1; f >= 0; --f) {
            if (f < fr.n && hit < 0 && fr.f[f].target == side) {
                int px, py;
                if (project_point(fr.f[f].P, fr.f[f].depth, px3, py3, pz3, px, py)) {
                    hit = f;
                    pix = py * fr.f[f].P.w + px;
                }
            }
        }
    }
    const int rows = n_points - base < kFramesPW ? (int)(n_points - base) : kFramesPW;
    for (int j = 0; j < rows; ++j) {
        const int fj = __builtin_amdgcn_readfirstlane(__shfl(hit, j, 64));
        const int pj = __builtin_amdgcn_readfirstlane(__shfl(pix, j, 64));
        float* __restrict__ dst = x + (base + j) * (long)ldx;
        if (fj < 0) {
            for (int ch = lane; ch < ldx; ch += 64) dst[ch] = ch <= c ? 1.0f : 0.0f;
            continue;
        }
        const float* fmap = fr.f[0].fmap;
        const float* valid = fr.f[0].valid;
        int h = fr.f[0].P.h, w = fr.f[0].P.w;
#pragma unroll
        for (int f = 1; f < kMaxFrames; ++f)
            if (fj == f) { fmap = fr.f[f].fmap; valid = fr.f[f].valid; h = fr.f[f].P.h; w = fr.f[f].P.w; }
        const int py = pj / w, px = pj - py * w;
        const float m = valid ? valid[(long)px * h + py] : 1.0f;      // valid is stored [w, h]
        const long plane = (long)h * w;
        const float* src = fmap + (long)py * w + px;
        for (int ch = lane; ch < ldx; ch += 64) dst[ch] = ch < c ? src[ch * plane] * m : (ch == c ? 1.0f : 0.0f);
    }
}

// numpy's basic-slice bounds for a[start:stop] on an axis of length len: negative counts from the end, then clamp
__device__ __forceinline__ int np_bound(long v, int len) {
    if (v < 0) v += len;
    if (v < 0) v = 0;
    if (v > len) v = len;
    return (int)v;
}
// int(k -/+ w) of a float32 keypoint coordinate: the exact value truncated toward zero (k -/+ w is exact in double, as in
// the reference's numpy float64 scalar arithmetic); coordinates beyond +-2^30 are clamped first (off any map either way)
__device__ __forceinline__ long trunc_coord(double v) {
    v = fmin(fmax(v, -1073741824.0), 1073741824.0);
    return (long)v;
}
__device__ __forceinline__ bool box_covers(float kx, float ky, int wnd, int mx, int my, int map_w, int map_h) {
    if (!(isfinite(kx) && isfinite(ky))) return false;
    const int x0 = np_bound(trunc_coord((double)kx - wnd), map_w), x1 = np_bound(trunc_coord((double)kx + wnd), map_w);
    const int y0 = np_bound(trunc_coord((double)ky - wnd), map_h), y1 = np_bound(trunc_coord((double)ky + wnd), map_h);
    return mx >= x0 && mx < x1 && my >= y0 && my < y1;
}

// one thread per (map, pixel): the last valid match whose box covers the pixel paints it (later matches overwrite earlier)
__global__ void __launch_bounds__(256) k_valid_maps(const float* __restrict__ kp0, const float* __restrict__ kp1, int n1,
                                                     const long long* __restrict__ matches, const float* __restrict__ conf,
                                                     int n0, int wnd, int map_w, int map_h, float* __restrict__ src_valid,
                                                     float* __restrict__ tgt_valid) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int side = blockIdx.y;
    if (e >= map_w * map_h) return;
    const int mx = e / map_h, my = e - mx * map_h;           // maps are [map_w, map_h]: first index the column x
    float v = 0.0f;
    for (int i = n0 - 1; i >= 0; --i) {
        const long long m = matches[i];
        if (m < 0 || m >= n1) continue;
        const float* a = kp0 + 2 * (long)i;
        const float* b = kp1 + 2 * m;
        if (!(isfinite(a[0]) && isfinite(a[1]) && isfinite(b[0]) && isfinite(b[1]))) continue;   // the MATCH paints nothing
        const float* k = side ? b : a;
        if (box_covers(k[0], k[1], wnd, mx, my, map_w, map_h)) {
            v = conf[i];
            break;
        }
    }
    (side ? tgt_valid : src_valid)[e] = v;
}

bool proj_params(const float* h_w2c, const float* h_K, float thresh, int h, int w, ProjParams& P) {
    if (!h_w2c || !h_K) return false;
    for (int k = 0; k < 16; ++k) {
        P.w2c.m[k] = h_w2c[k];
        P.K.m[k] = h_K[k];
    }
    P.thresh = thresh;
    P.h = h;
    P.w = w;
    return true;
}

}  // namespace
}  // namespace pcrcg

using namespace pcrcg;

extern "C" {

size_t pcrcg_project_depth_ws_bytes(int n) {
    if (n < 0) return 0;
    return carve_bytes((size_t)n, 4) * 2 + scan_ws_bytes(n);
}

int pcrcg_project_depth(const float* points, int n, const float* depth, int h, int w, const float* h_world2camera,
                        const float* h_intrinsics, float thresh, int64_t* inds2d, int64_t* inds3d, int* k, void* ws,
                        size_t ws_bytes, void* stream) {
    PCRCG_CHECK_ARG(n >= 0 && h >= 1 && w >= 1 && (long)h * w < (1L << 31));
    PCRCG_CHECK_ARG(depth && h_world2camera && h_intrinsics && k && ws);
    PCRCG_CHECK_ARG(n == 0 || (points && inds2d && inds3d));
    ProjParams P;
    proj_params(h_world2camera, h_intrinsics, thresh, h, w, P);
    Carver cv(ws, ws_bytes);
    int* flags = cv.take<int>((size_t)n);
    int* pix = cv.take<int>((size_t)n);
    void* scan_ws = cv.take<char>(scan_ws_bytes(n));
    PCRCG_CHECK_WS(cv);
    hipStream_t st = as_stream(stream);
    if (n == 0) {
        PCRCG_CHECK_HIP(hipMemsetAsync(k, 0, sizeof(int), st));
        return PCRCG_OK;
    }
    const unsigned g = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_project_flags, dim3(g), dim3(256), 0, st, points, n, depth, P, flags, pix);
    PCRCG_CHECK_LAUNCH();
    PCRCG_PROPAGATE(exclusive_scan_i32(flags, flags, n, k, scan_ws, st));
    hipLaunchKernelGGL(k_project_scatter, dim3(g), dim3(256), 0, st, pix, flags, n, w, reinterpret_cast<long long*>(inds2d),
                       reinterpret_cast<long long*>(inds3d));
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}

int pcrcg_inject_frames(const float* points, long n_points, long len_src, const pcrcg_image_frame* h_frames, int n_frames,
                        int c, float* x, int ldx, void* stream) {
    PCRCG_CHECK_ARG(n_points >= 0 && len_src >= 0 && len_src <= n_points && c >= 1 && ldx >= c + 1);
    PCRCG_CHECK_ARG(n_frames >= 0 && n_frames <= kMaxFrames && (n_frames == 0 || h_frames));
    Frames fr = {};
    int per_side[2] = {0, 0};
    for (int f = 0; f < n_frames; ++f) {
        const pcrcg_image_frame& F = h_frames[f];
        PCRCG_CHECK_ARG(F.fmap && F.depth && F.target >= 0 && F.target <= 1);
        PCRCG_CHECK_ARG(F.h >= 1 && F.w >= 1 && (long)F.h * F.w < (1L << 31));
        PCRCG_CHECK_ARG(F.depth_h == F.h && F.depth_w == F.w);
        PCRCG_CHECK_ARG(++per_side[F.target] <= 3);
        fr.f[f].fmap = F.fmap;
        fr.f[f].depth = F.depth;
        fr.f[f].valid = F.valid;
        fr.f[f].target = F.target;
        proj_params(F.world2camera, F.intrinsics, F.thresh, F.h, F.w, fr.f[f].P);
    }
    fr.n = n_frames;
    if (n_points == 0) return PCRCG_OK;
    PCRCG_CHECK_ARG(points && x);
    const long waves = (n_points + kFramesPW - 1) / kFramesPW;
    hipLaunchKernelGGL(k_inject_frames, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, as_stream(stream), points, n_points,
                       len_src, fr, c, x, ldx);
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}

int pcrcg_superglue_valid_maps(const float* keypoints0, int n0, const float* keypoints1, int n1, const int64_t* matches,
                               const float* confidence, int window, int map_w, int map_h, float* src_valid, float* tgt_valid,
                               void* stream) {
    PCRCG_CHECK_ARG(n0 >= 0 && n1 >= 0 && window >= 0 && map_w >= 1 && map_h >= 1 && (long)map_w * map_h < (1L << 31));
    PCRCG_CHECK_ARG(src_valid && tgt_valid);
    PCRCG_CHECK_ARG(n0 == 0 || (keypoints0 && matches && confidence));
    PCRCG_CHECK_ARG(n1 == 0 || keypoints1);
    const int px = map_w * map_h;
    hipLaunchKernelGGL(k_valid_maps, dim3((unsigned)((px + 255) / 256), 2), dim3(256), 0, as_stream(stream), keypoints0,
                       keypoints1, n1, reinterpret_cast<const long long*>(matches), confidence, n0, window, map_w,
                       map_h, src_valid, tgt_valid);
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}
}
