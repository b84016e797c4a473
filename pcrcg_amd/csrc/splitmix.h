// splitmix.h -- the counter-based generator shared by the RANSAC draws (register.hip) and the interest-point sampler
// (sample.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace pcrcg {

// splitmix64 (Steele, Lea & Flood 2014; the generator of java.util.SplittableRandom): the state x advanced by the golden
// gamma 0x9E3779B97F4A7C15, then the variant-13 finaliser.  include/pcrcg.h documents the same constants.
__host__ __device__ inline unsigned long long splitmix64(unsigned long long x) {
    unsigned long long z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

}  // namespace pcrcg
