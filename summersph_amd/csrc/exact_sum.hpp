// exact_sum.hpp -- the exact sums of pair_stats.hip (sph_pairs), history.hip (sph_history) and modes.hip (sph_modes): a
// term is formed in double, scaled by a power of two that a bound on the terms fixes, rounded half-even to a 64-bit integer
// and added into a 128-bit integer {lo, hi}; the total is converted to a double once.  Integer addition is associative, so
// a sum does not depend on the order, the launch or the shape of its reduction (DESIGN sections 26, 27 and 29).
#pragma once
#include <cmath>
#include <cstdint>

#include "sph_internal.hpp"

namespace sph {

// the exponent e with b < 2^e (b >= 0 and finite; 0 for b = 0)
__device__ __forceinline__ int32_t exp_above(double b) {
    int e = 0;
    (void)frexp(b, &e);
    return (int32_t)e;
}

// term 2^sh rounded half-even to an integer (|.| <= 2^62 by the bound that fixed sh)
__device__ __forceinline__ long long to_fixed(double term, int sh) { return (long long)rint(ldexp(term, sh)); }

// {lo, hi} += the sign-extended 64-bit t
__device__ __forceinline__ void add_fixed(unsigned long long &lo, unsigned long long &hi, long long t) {
    const unsigned long long tu = (unsigned long long)t;
    lo += tu;
    hi += (unsigned long long)(t >> 63) + (unsigned long long)(lo < tu);
}

// term 2^sh, rounded half-even to an integer, added into the 128-bit accumulator {h[0], h[1]} that other lanes add to as
// well (an LDS histogram): the low word with a returning add, the high word gets the term's sign word plus the carry the
// returned value shows
__device__ __forceinline__ void add_term(unsigned long long *h, double term, int sh) {
    const long long t = to_fixed(term, sh);
    const unsigned long long tu = (unsigned long long)t;
    const unsigned long long old = atomicAdd(h, tu);
    const long long up = (t >> 63) + (long long)(old + tu < old);
    if (up != 0) atomicAdd(h + 1, (unsigned long long)up);
}

// {lo, hi} += {l, h}
__device__ __forceinline__ void add_limbs(unsigned long long &lo, unsigned long long &hi, unsigned long long l,
                                          unsigned long long h) {
    lo += l;
    hi += h + (unsigned long long)(lo < l);
}

// the sum of {lo, hi} over the 64 lanes (xor butterfly of 128-bit additions): every lane ends with the same result
__device__ __forceinline__ void wave_add_limbs(unsigned long long &lo, unsigned long long &hi) {
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long l = __shfl_xor(lo, o, 64), h = __shfl_xor(hi, o, 64);
        add_limbs(lo, hi, l, h);
    }
}

// {lo, hi} 2^(e - 62), correctly rounded: the magnitude normalised to its top 64 bits with the rest as a sticky bit (the
// bits below a double's rounding position), then u64 -> f64 rounds half-even once, then an exact scaling
__device__ __forceinline__ double limbs_to_double(unsigned long long lo, unsigned long long hi, int e) {
    const bool neg = (long long)hi < 0;
    if (neg) {
        lo = ~lo + 1ull;
        hi = ~hi + (lo == 0ull);
    }
    if ((lo | hi) == 0ull) return 0.0;
    const int lz = hi ? __clzll((long long)hi) : 64 + __clzll((long long)lo);
    unsigned long long top, rest;
    if (lz >= 64) {
        top = lo << (lz - 64);
        rest = 0ull;
    } else if (lz == 0) {
        top = hi;
        rest = lo;
    } else {
        top = (hi << lz) | (lo >> (64 - lz));
        rest = lo << lz;
    }
    if (rest) top |= 1ull;
    const double d = ldexp((double)top, 64 - lz + e - 62);
    return neg ? -d : d;
}

// the same conversion on the host
inline double finish_one(uint64_t lo, uint64_t hi, int e) {
    const __int128 v = (__int128)(((unsigned __int128)hi << 64) | (unsigned __int128)lo);
    return std::ldexp((double)v, e - 62);                // int128 -> double rounds half-even once; the scaling is exact
}

}  // namespace sph
