// cellgrid.h -- the hashed uniform cell grid over a support set (pcrcg_cellgrid_build, radius.hip): workspace layout and
// the device helpers that walk it.  Shared by the radius search (radius.hip) and the registration back end (register.hip).
//
// A grid built with radius r has cells a hair wider than r (1 + 1e-5), so every support within r of a point lies in the
// 3 x 3 x 3 cells around the point's own.  Cloud b's open-addressing table is the 2 * len_b slots starting at slot
// 2 * (first support of b); a cell's supports are one contiguous run of spts, in no particular order within the run.
#pragma once
#include "common.h"

namespace pcrcg {
namespace {

typedef unsigned long long u64;
constexpr u64 kEmptyKey = ~0ull;
constexpr int kCoordBias = 1 << 20;   // cell coordinates are stored biased, 21 bits each

struct GridHeader {   // first 256 bytes of the grid workspace
    double inv_cell;  // 1 / (radius * (1 + 1e-5)): cells are a hair wider than the radius
    int ns, nb;
    u64 cursor;       // low word: bump allocator for cell runs; high word: occupied cells listed so far (ONE atomic)
    int overflow;     // coordinate range exceeded
};
constexpr int kTickStride = 64;       // ints between two ticket words: every counter in a 256-byte block of its own (eight
                                      // counters in ONE cache line were served one after the other, ~50 atomics per microsecond
                                      // for the whole chip: 84 of the 94 us of the 60 000-row search)

struct Slot {         // one 16-byte record per hash slot: a probe is ONE load
    u64 key;
    int cnt, start;
};

struct GridView {
    GridHeader* hdr;
    int* soff;     // [nb+1]
    Slot* tab;     // [2*ns + 2]
    int* slot_of;  // [ns]
    int* pos_in;   // [ns]
    float4* spts;  // [ns]  supports cell by cell as (x, y, z, index)
    u64* ckey;     // [ns]  occupied cells, compact (any order): key ...
    int4* cinfo;   // [ns]  ... and (count, start of the run in spts, cloud, slot)
    int* qtick;    // [16 * kTickStride]  k_radius_cells walking THIS grid as its query grid: ticket counter of shard k at
                   // [k * kTickStride], workgroups of shard k that have left at [(8 + k) * kTickStride]
};

inline size_t grid_bytes(int ns, int nb) {
    const size_t N = (size_t)(ns > 0 ? ns : 0) + 1;
    return carve_bytes(1, 256) + carve_bytes((size_t)nb + 1, sizeof(int)) + carve_bytes(2 * N, sizeof(Slot)) +
           2 * carve_bytes(N, sizeof(int)) + carve_bytes(N, sizeof(float4)) + carve_bytes(N, sizeof(u64)) +
           carve_bytes(N, sizeof(int4)) + carve_bytes(16 * kTickStride, sizeof(int));
}

inline GridView grid_view(void* ws, size_t bytes, int ns, int nb, bool* ok) {
    const size_t N = (size_t)(ns > 0 ? ns : 0) + 1;
    Carver cv(ws, bytes);
    GridView g;
    g.hdr = reinterpret_cast<GridHeader*>(cv.take<char>(256));
    g.soff = cv.take<int>((size_t)nb + 1);
    g.tab = cv.take<Slot>(2 * N);
    g.slot_of = cv.take<int>(N);
    g.pos_in = cv.take<int>(N);
    g.spts = cv.take<float4>(N);
    g.ckey = cv.take<u64>(N);
    g.cinfo = cv.take<int4>(N);
    g.qtick = cv.take<int>(16 * kTickStride);
    *ok = cv.ok();
    return g;
}

__device__ __forceinline__ Slot load_slot(const Slot* p) {     // one global_load_dwordx4
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    Slot s;
    s.key = (u64)v.x | ((u64)v.y << 32);
    s.cnt = (int)v.z;
    s.start = (int)v.w;
    return s;
}

__device__ __forceinline__ unsigned mix32(u64 x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
    return (unsigned)x;
}

// The cell of a float64 point: a point that was never an fp32 value (a source point moved in float64) must not be rounded to
// one first -- from about 100 m out half an fp32 ulp exceeds what a cell is wider than the radius by (4e-6 m at 0.0375 with the
// 1e-4 of correspondences.py), and the rounded point's 27 cells then miss targets the point's own 27 hold.
__device__ __forceinline__ bool cell_coords(double x, double y, double z, double inv_cell, int* cx, int* cy, int* cz) {
    const double fx = floor(x * inv_cell), fy = floor(y * inv_cell), fz = floor(z * inv_cell);
    const double lim = (double)(kCoordBias - 2);
    const bool ok = fx > -lim && fx < lim && fy > -lim && fy < lim && fz > -lim && fz < lim;
    *cx = ok ? (int)fx + kCoordBias : 0;
    *cy = ok ? (int)fy + kCoordBias : 0;
    *cz = ok ? (int)fz + kCoordBias : 0;
    return ok;
}
__device__ __forceinline__ bool cell_coords(float x, float y, float z, double inv_cell, int* cx, int* cy, int* cz) {
    return cell_coords((double)x, (double)y, (double)z, inv_cell, cx, cy, cz);
}
__device__ __forceinline__ u64 cell_key(int cx, int cy, int cz) {
    return (u64)(unsigned)cx | ((u64)(unsigned)cy << 21) | ((u64)(unsigned)cz << 42);
}

}  // namespace
}  // namespace pcrcg
