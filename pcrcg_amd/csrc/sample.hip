// sample.hip -- weighted sampling without replacement of interest points on gfx950: the step between the network's
// overlap x saliency scores and the registration back end.  ABI: include/pcrcg.h, section "Interest-point sampler".
//
// Replaces the host draw of ref:lib/tester.py:152-164 (np.random.choice(..., replace=False, p=scores / sum)) with a
// sampler of the same distribution that is specified on its own (tests/sample_ref.py restates it
// in numpy): row i of a segment with seed s gets the exponential-race key -log(u_i) / w_i (Efraimidis & Spirakis 2006),
// u_i from two rounds of splitmix64 on the counter (s << 40) + i, and the n rows with the smallest keys are kept, ties by
// ascending row, emitted in ascending row.
//
// One workgroup per segment, three phases over the segment's rows in strides of the workgroup:
//   keys      : float64 keys as their IEEE bit patterns (non-negative doubles order like unsigned integers) into the
//               workspace; thread t writes rows t, t + 1024, ... and is the only one that reads them again.
//   select    : the n-th smallest pattern by an MSB-first radix select, eight 8-bit passes with a 256-bin LDS histogram
//               (integer LDS atomics; a thread adds a run of equal bins at once, which is the whole first pass or two
//               since the leading exponent bits are shared).
//   compaction: chunks of 1024 rows in row order; one block scan of (below, equal) flags packed in one int places every
//               kept row -- those below the threshold and the first `need` rows equal to it -- at its rank.
// No floating-point atomics and no order that depends on the schedule: the result is a function of the segment's
// scores, n_keep and seed alone.  Compiled with -ffp-contract=off.
#include "block_scan.h"
#include "common.h"
#include "splitmix.h"

namespace pcrcg {
namespace {

typedef unsigned long long u64;

constexpr int kSampleThreads = 1024;
// domain constant of the sampler's stream ("SAMPLER1"): under one seed it is not the stream RANSAC draws its rows from
constexpr u64 kSampleDomain = 0x53414D504C455231ull;
constexpr u64 kInfBits = 0x7FF0000000000000ull;

// the key of row i as an orderable word; +inf for a score that is not a finite positive number
__device__ inline u64 sample_key(float w, u64 seed, int i) {
    if (!(w > 0.f) || w == INFINITY) return kInfBits;
    const u64 h = splitmix64(splitmix64((seed << 40) + (u64)i) ^ kSampleDomain);
    const double u = ((double)(h >> 11) + 0.5) * 0x1p-53;       // (0, 1]; 1 only for the single largest h >> 11
    const double key = -log(u) / (double)w;
    return (u64)__double_as_longlong(key) & 0x7FFFFFFFFFFFFFFFull;     // -0.0 (u = 1) orders as 0
}

__global__ void __launch_bounds__(kSampleThreads) k_weighted_sample(const float* __restrict__ scores, const int* __restrict__ seg_off,
                                                                    int n_keep, const u64* __restrict__ seeds,
                                                                    int* __restrict__ out_idx, const int* __restrict__ out_off,
                                                                    u64* __restrict__ keys, long cap) {
    __shared__ int s_hist[256];
    __shared__ int s_scan[kSampleThreads / 64];
    __shared__ int s_bin, s_need;
    const int seg = blockIdx.x, tid = threadIdx.x;
    const long r0 = seg_off[seg], r1 = seg_off[seg + 1];
    if (r0 < 0 || r1 <= r0 || r1 > cap) return;               // an empty segment, or offsets that leave the workspace
    const int N = (int)(r1 - r0);
    int* out = out_idx + out_off[seg];
    const u64 seed = seeds[seg];
    if (seed >= (1ull << 24)) {                                // not checkable on the host: the seeds live on the device
        for (int i = tid; i < min(N, n_keep); i += kSampleThreads) out[i] = -1;
        return;
    }
    if (N <= n_keep) {                                         // small clouds pass unchanged
        for (int i = tid; i < N; i += kSampleThreads) out[i] = i;
        return;
    }
    const float* w = scores + r0;
    u64* key = keys + r0;
    for (int i = tid; i < N; i += kSampleThreads) key[i] = sample_key(w[i], seed, i);

    // the n_keep-th smallest key: after pass p, `prefix` holds its leading 8 (p + 1) bits and `need` its rank among the
    // keys that share them
    u64 prefix = 0;
    int need = n_keep;
    for (int shift = 56; shift >= 0; shift -= 8) {
        if (tid < 256) s_hist[tid] = 0;
        __syncthreads();
        int run_bin = -1, run = 0;
        for (int i = tid; i < N; i += kSampleThreads) {
            const u64 k = key[i];
            if (shift < 56 && (k >> (shift + 8)) != prefix) continue;
            const int bin = (int)((k >> shift) & 255);
            if (bin != run_bin) {
                if (run) atomicAdd(&s_hist[run_bin], run);
                run_bin = bin;
                run = 0;
            }
            ++run;
        }
        if (run) atomicAdd(&s_hist[run_bin], run);
        __syncthreads();
        const int cnt = tid < 256 ? s_hist[tid] : 0;
        int total;
        const int before = block_excl_scan_i32<kSampleThreads>(cnt, &total, s_scan);
        if (tid < 256 && before < need && need <= before + cnt) {
            s_bin = tid;
            s_need = need - before;
        }
        __syncthreads();
        prefix = (prefix << 8) | (u64)s_bin;
        need = s_need;
    }
    // prefix = the threshold; kept: every row below it and the first `need` rows equal to it, in row order
    int done_eq = 0, done = 0;
    for (int base = 0; base < N; base += kSampleThreads) {
        const int i = base + tid;
        int lt = 0, eq = 0;
        if (i < N) {
            const u64 k = key[i];
            lt = k < prefix;
            eq = k == prefix;
        }
        int total;
        const int ex = block_excl_scan_i32<kSampleThreads>(lt | (eq << 16), &total, s_scan);
        const int eq_before = done_eq + (ex >> 16), lt_before = ex & 0xFFFF;
        if (lt || (eq && eq_before < need)) out[done + lt_before + min(eq_before, need) - min(done_eq, need)] = i;
        done += (total & 0xFFFF) + min(done_eq + (total >> 16), need) - min(done_eq, need);
        done_eq += total >> 16;
    }
}

}  // namespace
}  // namespace pcrcg

using namespace pcrcg;

extern "C" {

size_t pcrcg_weighted_sample_ws_bytes(int S, int n_total) {
    if (S < 1 || n_total < 0) return 0;
    return carve_bytes((size_t)(n_total > 0 ? n_total : 1), sizeof(u64));
}

int pcrcg_weighted_sample_batch(const float* scores, const int* seg_off, int S, int n_keep, const uint64_t* seeds, int* out_idx,
                                const int* out_off, void* ws, size_t ws_bytes, void* stream) {
    PCRCG_CHECK_ARG(scores && seg_off && seeds && out_idx && out_off && ws);
    PCRCG_CHECK_ARG(S >= 1 && n_keep >= 1);
    // the keys of every row; the kernel leaves a segment whose offsets do not lie inside them alone
    const long cap = (long)(ws_bytes / sizeof(u64));
    hipLaunchKernelGGL(k_weighted_sample, dim3(S), dim3(kSampleThreads), 0, as_stream(stream), scores, seg_off, n_keep,
                       reinterpret_cast<const u64*>(seeds), out_idx, out_off, static_cast<u64*>(ws), cap);
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}

}  // extern "C"
