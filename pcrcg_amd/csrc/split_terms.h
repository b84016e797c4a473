// split_terms.h -- the fp32 -> 16-bit term splits and the LDS operand row of the split-term MFMA products, shared by
// gemm_x6.hip (the GEMMs) and conv2d.hip (the implicit-GEMM 2-D convolutions).  Included inside namespace pcrcg's
// anonymous namespace of each file.
#pragma once

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

constexpr int ROWB = 80;   // bytes per LDS row of one plane: 32 bf16 + 16 B pad

// two fp32 -> their three bf16 terms, packed pairwise (low half = first element)
__device__ __forceinline__ void split2(float x0, float x1, unsigned& p1, unsigned& p2, unsigned& p3) {
    const unsigned u0 = __float_as_uint(x0), u1 = __float_as_uint(x1);
    const float h0 = __uint_as_float(u0 & 0xffff0000u), h1 = __uint_as_float(u1 & 0xffff0000u);
    const float r0 = x0 - h0, r1 = x1 - h1;                                   // exact
    const unsigned v0 = __float_as_uint(r0), v1 = __float_as_uint(r1);
    const float m0 = __uint_as_float(v0 & 0xffff0000u), m1 = __uint_as_float(v1 & 0xffff0000u);
    const float l0 = r0 - m0, l1 = r1 - m1;                                   // exact, <= 8 significant bits
    p1 = __builtin_amdgcn_perm(u1, u0, 0x07060302u);                          // {hi16(x1), hi16(x0)}
    p2 = __builtin_amdgcn_perm(v1, v0, 0x07060302u);
    p3 = __builtin_amdgcn_perm(__float_as_uint(l1), __float_as_uint(l0), 0x07060302u);
}

// The fp16 TWO-term form (H2 kernels): x = h + 2^-11 l with h = fp16_rn(x), l = fp16_rn((x - h) * 2^11) -- x - h is exact
// and at most half an ulp of h, so the scaled remainder is no larger than x and l loses nothing to the fp16 subnormal
// range that h did not.  |x - h - 2^-11 l| <= 2^-22 |x| (2^-36 absolute below 2^-14), and
//     a b = ha hb + 2^-11 (ha lb + la hb) + [2^-22 la lb]
// with the bracket and the representation error both at 2^-22 |ab|: three v_mfma_f32_32x32x16_f16 per 16-deep k-chunk
// (fp16 x fp16 products are exact in the matrix core's fp32 accumulation, fp16 subnormals are kept: scripts/micro/
// mfma_f16_denormal.hip) instead of six bf16 ones, two LDS planes instead of three, 4 instead of 11 VALU operations per
// operand pair.  Measured on the path's shapes: 4.5-5.8e-7 of a float64 product, a plain fp32 GEMM's error (the
// three-term bf16 form: 2.4e-7).  What the form cannot do is hold values outside fp16's NORMAL range, at either end:
// |x| >= 65520 becomes +-inf and leaves a non-finite partial sum behind; below 2^-14 h is a subnormal (below 2^-25: zero)
// and the split's error is an absolute 2^-36 instead of a relative 2^-22 -- harmless beside larger values of the same row,
// fatal for a row whose values are ALL that small.  Both are caught per tile after the loop (see the checks there), and a
// workgroup that finds either throws its sums away and runs its tile again with the three-term bf16 loop, which has fp32's
// range -- no flag for the host, no different result contract.
constexpr float kH2Scale = 2048.0f;          // 2^11
// Four VALU instructions per operand pair (round 5; the compiler's own code for the same arithmetic takes six): h by
// v_cvt_pk_f16_f32, y = 2^11 x by one packed multiply, and l = fp16_rn(y - 2^11 h) by the mixed-precision FMAs, which read
// h's halves as fp16 operands and round their (exact) fp32 result straight into the two halves of l.
// scripts/micro/split_mix.hip checks the pair bit for bit against the plain C++ form over random, subnormal and special values.
__device__ __forceinline__ void split2h(float x0, float x1, unsigned& p1, unsigned& p2) {
    const f32x2 x = {x0, x1};
    const f16x2 h = __builtin_convertvector(x, f16x2);                        // v_cvt_pk_f16_f32, round to nearest even
    const unsigned hb = __builtin_bit_cast(unsigned, h);
    const f32x2 y = x * kH2Scale;                                             // exact
    const float m = -kH2Scale;
    unsigned l;
    asm("v_fma_mixlo_f16 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(l) : "v"(hb), "s"(m), "v"(y[0]));
    asm("v_fma_mixhi_f16 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(l) : "v"(hb), "s"(m), "v"(y[1]));
    p1 = hb;
    p2 = l;
}
