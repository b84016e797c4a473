// hybrid_search.h -- open3d's hybrid neighbour search (radius and max_nn) of one point by one wavefront, over the hashed
// cell grid of cellgrid.h.  Shared by the normal estimation (normals.hip) and the FPFH descriptor (fpfh.hip); include/pcrcg.h
// "Normal estimation" defines the list.
//   probe   : lanes 0..26 look the 27 cells around the point up in its cloud's hash table (one 16-byte load per probe).
//   collect : the cells' supports are walked 64 at a time; a support with d2 < r2 (fp32, unfused) is appended to the
//             wavefront's LDS list.  Before the list could pass CAP entries it is ranked by (d2, index) and cut to its first
//             max_nn, so a cell neighbourhood of any size fits.  That needs max_nn + 64 <= CAP.  After a cut that filled
//             the list, a support farther than the list's last entry is dropped at once: max_nn nearer ones are known, so
//             it could not survive the next ranking (an equal d2 is kept: the index decides there).
//   rank    : the final list is ranked the same way: entry k is the k-th neighbour, whatever order the grid held them in.
// Files that include this are compiled with -ffp-contract=off.
#pragma once
#include "block_scan.h"
#include "cellgrid.h"
#include "common.h"

namespace pcrcg {
namespace {

template <int CAP>
struct HybridList {                               // one wavefront's candidates, twice: ranking writes the other copy
    float4 q[2][CAP];                             // (x, y, z, index)
    u64 key[2][CAP];                              // d2's bits (d2 >= +0: they order as d2 does) above the index: the rank order
};

__device__ __forceinline__ u64 hybrid_key(float d2, float4 q) {
    return ((u64)__float_as_uint(d2) << 32) | (u64)__float_as_uint(q.w);
}
__device__ __forceinline__ float hybrid_key_d2(u64 key) { return __uint_as_float((unsigned)(key >> 32)); }
template <int WAVES, int CAP>
struct HybridLds {
    HybridList<CAP> list[WAVES];
    int excl[WAVES][32];
    int start[WAVES][32];
};

// entries [0, fill) of copy `from` -> their first min(fill, keep) by (d2, index), in that order, in the other copy
template <int CAP>
__device__ __forceinline__ int rank_and_cut(HybridList<CAP>& l, int from, int fill, int keep, int lane) {
    for (int e = lane; e < fill; e += kWave) {
        const u64 mk = l.key[from][e];
        int rank = 0;
        for (int j = 0; j < fill; ++j) rank += l.key[from][j] < mk ? 1 : 0;          // keys are distinct: a permutation
        if (rank < keep) { l.key[from ^ 1][rank] = mk; l.q[from ^ 1][rank] = l.q[from][e]; }
    }
    __builtin_amdgcn_wave_barrier();
    return fill < keep ? fill : keep;
}

// The neighbour list of the point (px, py, pz) of cloud b, by the calling wavefront `wave` of its workgroup: -> its length k
// (<= max_nn); the entries are s.list[wave].q / .key [*cur][0, k), in (d2, index) order.
template <int WAVES, int CAP>
__device__ __forceinline__ int hybrid_search(HybridLds<WAVES, CAP>& s, int wave, int lane, float px, float py, float pz,
                                             const GridView& g, int b, float r2, int max_nn, int* cur_out) {
    HybridList<CAP>& l = s.list[wave];
    int cx, cy, cz;
    const bool inrange = cell_coords(px, py, pz, g.hdr->inv_cell, &cx, &cy, &cz);      // false for a NaN or far-away point
    const int first = g.soff[b], nsb = g.soff[b + 1] - first;
    const Slot* tab = g.tab + 2l * first;
    const unsigned tsize = nsb > 0 ? 2u * (unsigned)nsb : 0u;
    int ccount = 0, cstart = 0;
    if (lane < 27 && inrange && tsize > 0) {
        const u64 key = cell_key(cx + lane % 3 - 1, cy + (lane / 3) % 3 - 1, cz + lane / 9 - 1);
        unsigned sl_i = __umulhi(mix32(key), tsize);
        for (unsigned probe = 0; probe < tsize; ++probe) {
            const Slot sl = load_slot(&tab[sl_i]);
            if (sl.key == key) { ccount = sl.cnt; cstart = sl.start; break; }
            if (sl.key == kEmptyKey) break;
            sl_i = sl_i + 1 == tsize ? 0 : sl_i + 1;
        }
    }
    const int incl = wave_incl_scan_i32(ccount, lane);
    const int total = __shfl(incl, 26, kWave);
    if (lane < 32) { s.excl[wave][lane] = lane < 27 ? incl - ccount : 0x7FFFFFFF; s.start[wave][lane] = cstart; }
    __builtin_amdgcn_wave_barrier();

    int cur = 0, fill = 0;
    float last = __int_as_float(0x7f800000);      // once a cut has filled the list: its last d2; a farther hit cannot get in
    for (int base = 0; base < total; base += kWave) {
        if (fill > CAP - kWave) {                 // the next 64 might not fit: keep the best max_nn of what is there
            fill = rank_and_cut(l, cur, fill, max_nn, lane);
            cur ^= 1;
            if (fill == max_nn) last = hybrid_key_d2(l.key[cur][max_nn - 1]);
        }
        const int t = base + lane;
        const int tc = t < total ? t : total - 1;
        int lo = 0;
#pragma unroll
        for (int step = 16; step >= 1; step >>= 1)
            if (s.excl[wave][lo + step] <= tc) lo += step;
        const float4 q = g.spts[s.start[wave][lo] + (tc - s.excl[wave][lo])];
        const float dx = q.x - px, dy = q.y - py, dz = q.z - pz;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        const bool hit = t < total && d2 < r2 && d2 <= last;
        const u64 mask = __ballot(hit);
        const int pos = fill + __popcll(mask & ((1ull << lane) - 1ull));
        if (hit) { l.key[cur][pos] = hybrid_key(d2, q); l.q[cur][pos] = q; }          // pos < fill + 64 <= CAP
        fill += __popcll(mask);
        __builtin_amdgcn_wave_barrier();
    }
    const int k = rank_and_cut(l, cur, fill, max_nn, lane);
    *cur_out = cur ^ 1;
    return k;
}

}  // namespace
}  // namespace pcrcg
