// fpfh.hip -- FPFH descriptors of B ragged clouds on gfx950: the classical 33-bin descriptor that feeds feature matching and
// RANSAC (register.hip) without the network.
// ABI: include/pcrcg.h, section "FPFH descriptors"; DESIGN.md section 21 defines the algorithm and tests/fpfh_ref.py restates
// it in numpy.
//
// open3d's ComputeFPFHFeature(KDTreeSearchParamHybrid(radius, max_nn)), restated, in two launches; one wavefront per point in
// both.
//   k_fpfh_spfh : the search of hybrid_search.h with a list of 192 entries (up to 128 kept + 64 of the current step); lane e
//                 and lane e + 64 take list entries e and e + 64, compute their pair features in float64 and count them into
//                 the wavefront's 33 integer bins in LDS (integer adds: exact and order-free).  It stores the histogram as
//                 bytes (a bin holds at most 127), the list's length and the ordered list of neighbour rows.
//   k_fpfh_sum  : reads the stored list back -- the search is the expensive part, and the list is 4 bytes per entry beside
//                 the 36 the gather reads.  Lanes compute D and 100 / (k_q - 1) of two entries each, the wavefront copies
//                 the neighbours' byte histograms to LDS with independent 4-byte loads, and lane j < 33 then adds bin j over
//                 the entries in list order, normalises its group of 11 and adds the point's own SPFH.
// Nothing is added by floating-point atomics: a row's bits depend on its cloud's points and normals alone.
//
// Compiled with -ffp-contract=off (every operation rounds where the source says).
#include "common.h"
#include "hybrid_search.h"

namespace pcrcg {
namespace {

constexpr int kFpfhWaves = 4;                     // points per workgroup
constexpr int kFpfhMaxNn = 128;                   // two list entries per lane
constexpr int kFpfhCap = kFpfhMaxNn + kWave;      // list entries per wavefront: up to 128 kept + 64 of the current step
constexpr int kFpfhBins = 33;
constexpr int kFpfhRowWords = 9;                  // a stored histogram: 33 bytes padded to 36, read as nine words
constexpr int kFpfhMaxBatch = 65535;              // clouds ride on a grid dimension

struct FpfhWs {
    int* k;                // [n_total]                the lists' lengths
    unsigned* hist;        // [n_total, 9]             byte histograms, 33 bytes + 3 of padding per row
    int* nbr;              // [n_total, max_nn]        the ordered lists: rows of pts
};

struct FpfhArgs {
    const float* pts;
    const int* off;
    const double* normals;      // [n_total, 3]
    float* fpfh;                // [n_total, 33]
    int* count;                 // [n_total] or null
    unsigned char* hist;        // [n_total, 33] or null
    double* fpfh64;             // [n_total, 33] or null
    FpfhWs ws;
    float r2;
    int max_nn;
};

struct SpfhLds {
    HybridLds<kFpfhWaves, kFpfhCap> srch;
    int bins[kFpfhWaves][kFpfhRowWords * 4];
};

// The pair feature of (p, n1) with (q, n2) -> its three bins (each 0..10) as h0 | h1 << 8 | h2 << 16; -1 if a feature is not
// finite.
__device__ __forceinline__ int pair_bins(double px, double py, double pz, double n1x, double n1y, double n1z, double qx,
                                          double qy, double qz, double n2x, double n2y, double n2z) {
    double dx = qx - px, dy = qy - py, dz = qz - pz;
    const double d = sqrt((dx * dx + dy * dy) + dz * dz);
    double f0 = 0.0, f1 = 0.0, f2 = 0.0;
    if (d != 0.0) {
        const double a1 = ((n1x * dx + n1y * dy) + n1z * dz) / d;
        const double a2 = ((n2x * dx + n2y * dy) + n2z * dz) / d;
        if (fabs(a1) < fabs(a2)) {
            double t;
            t = n1x; n1x = n2x; n2x = t;
            t = n1y; n1y = n2y; n2y = t;
            t = n1z; n1z = n2z; n2z = t;
            dx = -dx; dy = -dy; dz = -dz;
            f2 = -a2;
        } else {
            f2 = a1;
        }
        double vx = dy * n1z - dz * n1y, vy = dz * n1x - dx * n1z, vz = dx * n1y - dy * n1x;      // dp x n1
        const double vn = sqrt((vx * vx + vy * vy) + vz * vz);
        if (vn != 0.0) {
            vx = vx / vn; vy = vy / vn; vz = vz / vn;
            const double wx = n1y * vz - n1z * vy, wy = n1z * vx - n1x * vz, wz = n1x * vy - n1y * vx;   // n1 x v
            f1 = (vx * n2x + vy * n2y) + vz * n2z;
            f0 = atan2((wx * n2x + wy * n2y) + wz * n2z, (n1x * n2x + n1y * n2y) + n1z * n2z);
        } else {
            f2 = 0.0;
        }
    }
    if (!(isfinite(f0) && isfinite(f1) && isfinite(f2))) return -1;
    const double b0 = floor(11.0 * (f0 + M_PI) / (2.0 * M_PI));
    const double b1 = floor(11.0 * (f1 + 1.0) * 0.5);
    const double b2 = floor(11.0 * (f2 + 1.0) * 0.5);
    return (int)fmin(fmax(b0, 0.0), 10.0) | ((int)fmin(fmax(b1, 0.0), 10.0) << 8) | ((int)fmin(fmax(b2, 0.0), 10.0) << 16);
}

// grid (blocks of four rows, cloud)
__global__ void __launch_bounds__(kFpfhWaves* kWave) k_fpfh_spfh(FpfhArgs a, GridView g) {
    __shared__ SpfhLds s;
    const int lane = threadIdx.x & (kWave - 1), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const int b = blockIdx.y;
    const int i0 = a.off[b], n = a.off[b + 1] - i0;
    const int il = blockIdx.x * kFpfhWaves + wave;
    if (il >= n) return;
    const long i = (long)i0 + il;
    const float px = a.pts[3 * i], py = a.pts[3 * i + 1], pz = a.pts[3 * i + 2];
    const HybridList<kFpfhCap>& l = s.srch.list[wave];
    int cur;
    const int k = hybrid_search(s.srch, wave, lane, px, py, pz, g, b, a.r2, a.max_nn, &cur);     // k <= max_nn <= 128

    int* bins = s.bins[wave];
    if (lane < kFpfhRowWords * 4) bins[lane] = 0;
    __builtin_amdgcn_wave_barrier();
    const double n1x = a.normals[3 * i], n1y = a.normals[3 * i + 1], n1z = a.normals[3 * i + 2];
    int* list = a.ws.nbr + (size_t)i * (size_t)a.max_nn;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int e = lane + half * kWave;
        if (e < k) {
            const float4 q = l.q[cur][e];
            const int row = __float_as_int(q.w);
            list[e] = row;
            if (e >= 1) {                         // entry 0 is skipped
                const double* n2 = a.normals + 3l * row;
                const int h = pair_bins((double)px, (double)py, (double)pz, n1x, n1y, n1z, (double)q.x, (double)q.y, (double)q.z,
                                        n2[0], n2[1], n2[2]);
                if (h >= 0) {
                    atomicAdd(&bins[h & 255], 1);
                    atomicAdd(&bins[11 + ((h >> 8) & 255)], 1);
                    atomicAdd(&bins[22 + (h >> 16)], 1);
                }
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < kFpfhRowWords) {                   // bins 33..35 stay zero: the padding
        const unsigned w = (unsigned)bins[4 * lane] | ((unsigned)bins[4 * lane + 1] << 8) | ((unsigned)bins[4 * lane + 2] << 16) |
                           ((unsigned)bins[4 * lane + 3] << 24);
        a.ws.hist[(size_t)i * kFpfhRowWords + lane] = w;
    }
    if (lane < kFpfhBins && a.hist) a.hist[(size_t)i * kFpfhBins + lane] = (unsigned char)bins[lane];
    if (lane == 0) {
        a.ws.k[i] = k;
        if (a.count) a.count[i] = k;
    }
}

struct SumLds {
    unsigned rows[kFpfhWaves][kFpfhMaxNn * kFpfhRowWords];       // the list members' byte histograms
    double D[kFpfhWaves][kFpfhMaxNn];
    double incr[kFpfhWaves][kFpfhMaxNn];
    double F[kFpfhWaves][kFpfhBins];
    int row[kFpfhWaves][kFpfhMaxNn];
};

// grid (blocks of four rows, cloud)
__global__ void __launch_bounds__(kFpfhWaves* kWave) k_fpfh_sum(FpfhArgs a) {
    __shared__ SumLds s;
    const int lane = threadIdx.x & (kWave - 1), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const int b = blockIdx.y;
    const int i0 = a.off[b], n = a.off[b + 1] - i0;
    const int il = blockIdx.x * kFpfhWaves + wave;
    if (il >= n) return;
    const long i = (long)i0 + il;
    const int k = __builtin_amdgcn_readfirstlane(a.ws.k[i]);
    const int j = lane < kFpfhBins ? lane : kFpfhBins - 1;        // lanes 33..63 shadow bin 32 and store nothing
    float* o32 = a.fpfh + (size_t)i * kFpfhBins;
    double* o64 = a.fpfh64 ? a.fpfh64 + (size_t)i * kFpfhBins : nullptr;
    if (k <= 1) {
        if (lane < kFpfhBins) {
            o32[lane] = 0.0f;
            if (o64) o64[lane] = 0.0;
        }
        return;
    }
    const double px = (double)a.pts[3 * i], py = (double)a.pts[3 * i + 1], pz = (double)a.pts[3 * i + 2];
    const int* list = a.ws.nbr + (size_t)i * (size_t)a.max_nn;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int e = lane + half * kWave;
        if (e < k) {
            const int row = list[e];
            const double dx = (double)a.pts[3l * row] - px, dy = (double)a.pts[3l * row + 1] - py,
                         dz = (double)a.pts[3l * row + 2] - pz;
            const int kq = a.ws.k[row];
            s.row[wave][e] = row;
            s.D[wave][e] = (dx * dx + dy * dy) + dz * dz;
            s.incr[wave][e] = kq > 1 ? 100.0 / (double)(kq - 1) : 0.0;
        }
    }
    __builtin_amdgcn_wave_barrier();
    for (int t = lane; t < k * kFpfhRowWords; t += kWave) {       // t < 128 * 9: inside rows[wave]
        const int e = t / kFpfhRowWords;
        s.rows[wave][t] = a.ws.hist[(size_t)s.row[wave][e] * kFpfhRowWords + (t - e * kFpfhRowWords)];
    }
    __builtin_amdgcn_wave_barrier();

    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(s.rows[wave]);
    double F = 0.0;
    for (int e = 1; e < k; ++e) {
        const double D = s.D[wave][e];
        if (D == 0.0) continue;                                   // the same in every lane
        const double spfh = (double)bytes[e * (kFpfhRowWords * 4) + j] * s.incr[wave][e];
        F = F + spfh / D;
    }
    if (lane < kFpfhBins) s.F[wave][lane] = F;
    __builtin_amdgcn_wave_barrier();
    const int g0 = 11 * (j / 11);
    double S = 0.0;
#pragma unroll
    for (int t = 0; t < 11; ++t) S = S + s.F[wave][g0 + t];
    if (S != 0.0) F = F * (100.0 / S);
    const unsigned own = a.ws.hist[(size_t)i * kFpfhRowWords + j / 4];
    const double c = (double)((own >> (8 * (j & 3))) & 255u);
    const double out = F + c * (100.0 / (double)(k - 1));
    if (lane < kFpfhBins) {
        o32[lane] = (float)out;
        if (o64) o64[lane] = out;
    }
}

FpfhWs carve_fpfh(Carver& cv, int n_total, int max_nn) {
    const size_t N = (size_t)n_total + 1;
    FpfhWs w;
    w.k = cv.take<int>(N);
    w.hist = cv.take<unsigned>(N * kFpfhRowWords);
    w.nbr = cv.take<int>(N * (size_t)max_nn);
    return w;
}

}  // namespace
}  // namespace pcrcg

using namespace pcrcg;

extern "C" {

size_t pcrcg_fpfh_ws_bytes(int B, int n_total, int max_nn) {
    if (B < 1 || B > kFpfhMaxBatch || n_total < 0 || max_nn < 1 || max_nn > kFpfhMaxNn) return 0;
    const size_t N = (size_t)n_total + 1;                                   // what carve_fpfh takes
    return carve_bytes(N, sizeof(int)) + carve_bytes(N * kFpfhRowWords, sizeof(unsigned)) +
           carve_bytes(N * (size_t)max_nn, sizeof(int));
}

int pcrcg_fpfh_batch(const float* pts, const int* off, int n_total, int n_max, const void* grid, int B, double radius, int max_nn,
                     const double* normals, float* fpfh, int* count, unsigned char* hist, double* fpfh64, void* ws,
                     size_t ws_bytes, void* stream) {
    PCRCG_CHECK_ARG(off && grid && ws);
    PCRCG_CHECK_ARG(B >= 1 && B <= kFpfhMaxBatch);
    PCRCG_CHECK_ARG(n_total >= 0 && n_max >= 0 && n_max <= n_total);
    PCRCG_CHECK_ARG(n_total == 0 || (pts && normals && fpfh));
    PCRCG_CHECK_ARG(radius > 0.0 && radius < 1e18);                         // (false for a NaN)
    PCRCG_CHECK_ARG(max_nn >= 1 && max_nn <= kFpfhMaxNn);
    Carver cv(ws, ws_bytes);
    FpfhArgs a;
    a.ws = carve_fpfh(cv, n_total, max_nn);
    PCRCG_CHECK_WS(cv);
    if (n_max == 0) return PCRCG_OK;
    bool ok;
    GridView g = grid_view(const_cast<void*>(grid), grid_bytes(n_total, B), n_total, B, &ok);
    a.pts = pts; a.off = off; a.normals = normals;
    a.fpfh = fpfh; a.count = count; a.hist = hist; a.fpfh64 = fpfh64;
    a.r2 = (float)radius * (float)radius;
    a.max_nn = max_nn;
    const dim3 blocks((n_max + kFpfhWaves - 1) / kFpfhWaves, B), threads(kFpfhWaves * kWave);
    hipLaunchKernelGGL(k_fpfh_spfh, blocks, threads, 0, as_stream(stream), a, g);
    PCRCG_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_fpfh_sum, blocks, threads, 0, as_stream(stream), a);
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}

}  // extern "C"
