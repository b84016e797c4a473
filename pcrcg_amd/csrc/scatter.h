// scatter.h -- the accumulation the scatter kernels share (trainops.hip; kpconv_ex.hip's backward): fp32 atomics by default,
// fixed-point integer sums under PCRCG_DEBUG=deterministic=1 (include/pcrcg.h).  The host side (det_begin / det_end, the
// per-stream scratch) is in trainops.hip.
#pragma once
#include <type_traits>

#include "common.h"

namespace pcrcg {

// ---- deterministic accumulation (PCRCG_DEBUG=deterministic=1, include/pcrcg.h) ----------------------------------------
// The scatter kernels add into a support row from many queries at once; with fp32 atomics the order of those adds --
// and so the last bits of the result -- changes from run to run.  Integer addition is associative: under the switch every
// contribution is rounded ONCE to 64-bit fixed point (scale 2^S, S chosen on the device from the largest magnitude of the
// source gradient so that 2^22 contributions cannot overflow: resolution 2^-39 of that magnitude, finer than fp32) and added
// with a 64-bit integer atomic into a zeroed scratch buffer of the destination's shape; k_fix_flush then adds the exact
// integer sums to the destination (one fp32 rounding per element) and leaves the scratch zeroed for the next use.  The
// scratch is the library's own (one buffer per stream, grown on demand): a debugging mode pays for its memory itself.
struct FixAcc {
    long long* acc;            // NULL: plain fp32 atomics (the default)
    const unsigned* maxbits;   // bit pattern of the largest |source gradient| (k_absmax_bits)
    int fan_log2;              // log2 of (contributions per element x the largest factor a contribution carries)
    const unsigned* factorbits;  // NULL, or the bit pattern of the largest per-channel factor a contribution carries
                                 // beyond the source gradient (edge conv: rstd), which then joins the magnitude
};
// An all-zero source gradient (maxbits == 0: e.g. an output nobody differentiated) has nothing to add: scale 0, every
// contribution rounds to the integer 0 and the flush skips its (still zero) sums.  The scale is a power of two held in
// double: gradients down to fp32's subnormals keep the full 2^-(62 - fan_log2) resolution (an fp32 scale would have to
// clamp its exponent at 126 -- ~1e-3 relative below magnitudes of 1e-26).  A contribution times the scale is exact in
// double, so it rounds to the same integer as the fp32 product did wherever that product stayed in range.
__device__ __forceinline__ double fix_scale(const FixAcc& f) {
    const unsigned bits = *f.maxbits;
    if (bits == 0u) return 0.0;
    int e1 = (int)((bits >> 23) & 0xff) - 126;                     // largest magnitude < 2^e1
    if (f.factorbits) {
        const unsigned fb = *f.factorbits;
        if (fb == 0u) return 0.0;
        e1 += (int)((fb >> 23) & 0xff) - 126;
    }
    return ldexp(1.0, 62 - f.fan_log2 - e1);
}
template <bool DET>
__device__ __forceinline__ void scatter_add(float* dst, long off, float v, const FixAcc& f, double scale) {
    if constexpr (DET) atomicAdd(reinterpret_cast<unsigned long long*>(f.acc) + off, (unsigned long long)__double2ll_rn((double)v * scale));
    else atomicAdd(dst + off, v);
}

// ---- the host side (trainops.hip) -----------------------------------------------------------------------------------------
struct FView { const float* p = nullptr; long rows = 0; int cols = 0; long ld = 0; };   // rows x cols values, row r at p + r * ld
// -> a FixAcc over a zeroed buffer of at least `elems` elements whose scale follows the largest |src| value (times the largest
// |factor| value when one is given)
int det_begin(hipStream_t st, size_t elems, const FView& src, int fan_log2, const FView& factor, FixAcc* out);
int det_end(hipStream_t st, const FixAcc& fx, float* dst, size_t elems);

// One scatter into dst [elems], in the mode the library is in.  launch(det, fx) enqueues the scatter kernel(s) instantiated
// with decltype(det)::value: fp32 atomics onto dst (the default), or -- deterministic=1 -- fixed-point sums of the
// contributions of `src` (each carrying at most 2^fan_log2 x the largest |factor|) that det_end then adds to dst.  Every
// kernel's argument list is written once, for both modes.
template <typename Launch>
int scatter_launch(hipStream_t st, size_t elems, const FView& src, int fan_log2, const FView& factor, float* dst, Launch launch) {
    if (debug_opts().deterministic) {
        FixAcc fx;
        PCRCG_PROPAGATE(det_begin(st, elems, src, fan_log2, factor, &fx));
        launch(std::true_type(), fx);
        PCRCG_CHECK_LAUNCH();
        return det_end(st, fx, dst, elems);
    }
    launch(std::false_type(), FixAcc{nullptr, nullptr, 0, nullptr});
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}

}  // namespace pcrcg
