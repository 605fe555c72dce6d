// af_wide.hpp -- fixed-width unsigned integers of 256 bits for the analyzers whose results are exact integers wider than a
// machine word (af_series_warmup.hpp).  A value is four 64-bit limbs, low limb first; every operation is modulo 2^256 and says
// so -- the callers state the width contract under which nothing wraps.  AF_HD functions without a HIP include, as af_math.hpp:
// the same text is gfx950 device code and, under g++, the host instantiation that tests/hostcheck/warmup_check.cpp runs
// against Python integers.  No floating point, no division, no branch on the data but the compare.
#pragma once

#include <stdint.h>

#if !defined(AF_HD)
#if defined(__HIPCC__)
#define AF_HD __host__ __device__ __forceinline__
#else
#define AF_HD inline
#endif
#endif

namespace afw256 {

struct U256 {
    uint64_t w[4];   // w[0] the low limb
};

AF_HD U256 zero() { return U256{{0ull, 0ull, 0ull, 0ull}}; }
AF_HD U256 from_u64(uint64_t v) { return U256{{v, 0ull, 0ull, 0ull}}; }
AF_HD U256 from_u128(uint64_t lo, uint64_t hi) { return U256{{lo, hi, 0ull, 0ull}}; }

// a * b as (low, high) words
AF_HD uint64_t mul64(uint64_t a, uint64_t b, uint64_t& hi) {
    const unsigned __int128 p = (unsigned __int128)a * b;
    hi = (uint64_t)(p >> 64);
    return (uint64_t)p;
}

// a + b + carry-in (0 or 1); the carry out comes back in `carry`
AF_HD uint64_t addc(uint64_t a, uint64_t b, uint64_t& carry) {
    const uint64_t s = a + b;
    const uint64_t c1 = s < a ? 1ull : 0ull;
    const uint64_t t = s + carry;
    carry = c1 | (t < s ? 1ull : 0ull);   // (at most one of the two additions wraps)
    return t;
}

// a - b - borrow-in (0 or 1); the borrow out comes back in `borrow`
AF_HD uint64_t subb(uint64_t a, uint64_t b, uint64_t& borrow) {
    const uint64_t d = a - b;
    const uint64_t b1 = a < b ? 1ull : 0ull;
    const uint64_t t = d - borrow;
    borrow = b1 | (d < borrow ? 1ull : 0ull);
    return t;
}

// (a + b) mod 2^256
AF_HD U256 add(const U256& a, const U256& b) {
    U256 r;
    uint64_t c = 0ull;
#pragma unroll
    for (int i = 0; i < 4; ++i) r.w[i] = addc(a.w[i], b.w[i], c);
    return r;
}

// (a + v) mod 2^256
AF_HD U256 add_u64(const U256& a, uint64_t v) { return add(a, from_u64(v)); }

// (a - b) mod 2^256: a - b where a >= b
AF_HD U256 sub(const U256& a, const U256& b) {
    U256 r;
    uint64_t c = 0ull;
#pragma unroll
    for (int i = 0; i < 4; ++i) r.w[i] = subb(a.w[i], b.w[i], c);
    return r;
}

// (a * k) mod 2^256
AF_HD U256 mul_u64(const U256& a, uint64_t k) {
    U256 r;
    uint64_t carry = 0ull;   // the high word of the limb below (plus its carry: < 2^64, as (2^64 - 1)^2 + 2^64 - 1 < 2^128)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint64_t hi;
        const uint64_t lo = mul64(a.w[i], k, hi);
        r.w[i] = lo + carry;
        carry = hi + (r.w[i] < lo ? 1ull : 0ull);
    }
    return r;
}

// the widening multiply: (a * (k_hi * 2^64 + k_lo)) mod 2^256.  Exact whenever the product is below 2^256: a 178-bit A times a
// 75-bit m^3, or an 89-bit S1 times itself.
AF_HD U256 mul_u128(const U256& a, uint64_t k_lo, uint64_t k_hi) {
    const U256 low = mul_u64(a, k_lo);
    const U256 high = mul_u64(a, k_hi);
    U256 r;
    r.w[0] = low.w[0];
    uint64_t c = 0ull;
#pragma unroll
    for (int i = 1; i < 4; ++i) r.w[i] = addc(low.w[i], high.w[i - 1], c);
    return r;
}

// -1, 0, 1 as a < b, a == b, a > b
AF_HD int cmp(const U256& a, const U256& b) {
    int r = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) r = a.w[i] < b.w[i] ? -1 : (a.w[i] > b.w[i] ? 1 : r);   // (a higher limb overrules the lower ones)
    return r;
}

}  // namespace afw256
