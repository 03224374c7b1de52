// quantile_plan.hpp — geometry and arithmetic of the ring quantiles: per sampled tick and component element, exact order statistics
// over the finite rows of one group (row % period).  Pure arithmetic, no HIP: the kernels (quantile_kernels.hip) and the host twin
// (hip_fake.cpp) run the same functions, sixdof_history_quantiles (sixdof_capi.cpp) sizes its buffers with them,
// quantile_host_test.cpp checks them on the host.
//
// Selection is a radix select, most significant digit first, over an order-preserving integer key: per pass and (bin, rank) a
// histogram of the next 8-bit digit over the elements whose higher digits equal the rank's prefix so far, a scan of it that
// picks the digit holding the rank, and the rank reduced by the count below.  After the last pass the prefix is the key of
// x(lo); x(hi) is the same element or the smallest key above it.  Ranks are exact rationals: no floating-point arithmetic.
//
// One tick of one component is a matrix of n / period rows by bins = period * w columns (element i in bin i % bins, as in
// envelope_plan.hpp).  A block keeps the histograms of all ranks of `cols` consecutive bins in LDS; where bins * ranks exceeds
// what LDS holds the bins are split over blocks, each of which reads its columns only.
#pragma once

#include <cstdint>

#include "envelope_plan.hpp"

namespace sixdof {

constexpr uint32_t kQuantileThreads = 512;       // threads of a pass block
constexpr uint32_t kQuantileMaxRanks = 16;       // SIXDOF_QUANTILE_MAX_RANKS
constexpr uint32_t kQuantileDigitBits = 8;
constexpr uint32_t kQuantileDigits = 1u << kQuantileDigitBits;
constexpr uint32_t kQuantileBlockSlots = 48;     // (bin, rank) histograms a block keeps in LDS: 48 KiB
constexpr uint32_t kQuantileMaxRowBlocks = 32;   // blocks that share the rows of one column range
constexpr uint32_t kQuantileSweepsPerBlock = 4;  // fewer blocks rather than blocks with less than this to read

// ---- the key: unsigned order == the total order of sign-magnitude floats (-0.0 below +0.0) ---------------------------------
SIXDOF_HOST_DEVICE inline uint64_t quantile_key64(uint64_t u) { return u ^ ((u >> 63) ? ~uint64_t(0) : uint64_t(1) << 63); }
SIXDOF_HOST_DEVICE inline uint32_t quantile_key32(uint32_t u) { return u ^ ((u >> 31) ? ~uint32_t(0) : uint32_t(1) << 31); }
SIXDOF_HOST_DEVICE inline uint64_t quantile_unkey64(uint64_t k) { return (k >> 63) ? k ^ (uint64_t(1) << 63) : ~k; }
SIXDOF_HOST_DEVICE inline uint32_t quantile_unkey32(uint32_t k) { return (k >> 31) ? k ^ (uint32_t(1) << 31) : ~k; }

// An element type's bit pattern, finiteness and key; keys of both types are carried in 64 bits (f32: the low 32).
template <class E> struct QuantileBits;
template <> struct QuantileBits<double> {
    static constexpr uint32_t bits = 64;
    SIXDOF_HOST_DEVICE static uint64_t raw(double x) { uint64_t u; __builtin_memcpy(&u, &x, 8); return u; }
    SIXDOF_HOST_DEVICE static bool finite(uint64_t u) { return (u & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }
    SIXDOF_HOST_DEVICE static uint64_t key(uint64_t u) { return quantile_key64(u); }
    SIXDOF_HOST_DEVICE static double value(uint64_t key) { const uint64_t u = quantile_unkey64(key); double x; __builtin_memcpy(&x, &u, 8); return x; }
};
template <> struct QuantileBits<float> {
    static constexpr uint32_t bits = 32;
    SIXDOF_HOST_DEVICE static uint64_t raw(float x) { uint32_t u; __builtin_memcpy(&u, &x, 4); return u; }
    SIXDOF_HOST_DEVICE static bool finite(uint64_t u) { return (u & 0x7f800000u) != 0x7f800000u; }
    SIXDOF_HOST_DEVICE static uint64_t key(uint64_t u) { return quantile_key32(static_cast<uint32_t>(u)); }
    SIXDOF_HOST_DEVICE static double value(uint64_t key) { const uint32_t u = quantile_unkey32(static_cast<uint32_t>(key)); float x; __builtin_memcpy(&x, &u, 4); return static_cast<double>(x); }
};
SIXDOF_HOST_DEVICE inline uint32_t quantile_passes(uint32_t key_bits) { return key_bits / kQuantileDigitBits; }
// pass p looks at the digit at this shift, among the elements whose bits above it (the mask) equal the prefix
SIXDOF_HOST_DEVICE inline uint32_t quantile_shift(uint32_t key_bits, uint32_t pass) { return key_bits - kQuantileDigitBits * (pass + 1); }
SIXDOF_HOST_DEVICE inline uint64_t quantile_prefix_mask(uint32_t key_bits, uint32_t pass) {
    return pass == 0 ? 0 : ~uint64_t(0) << (quantile_shift(key_bits, pass) + kQuantileDigitBits);
}
SIXDOF_HOST_DEVICE inline uint32_t quantile_digit(uint64_t key, uint32_t shift) { return static_cast<uint32_t>(key >> shift) & (kQuantileDigits - 1); }

// ---- ranks ------------------------------------------------------------------------------------------------------------
struct QuantileRanks {   // by value into the kernels
    uint32_t num[kQuantileMaxRanks];
    uint32_t den, count;
};
// What launch_history_quantiles accepts, for the launcher (quantile_kernels.hip) and its host twin (hip_fake.cpp) alike: the
// envelope's limits, whole groups whose rows a 32-bit counter holds, 1 to 16 ranks over a denominator.
inline bool quantile_launch_ok(uint32_t n_components, uint32_t max_components, const QuantileRanks& ranks, uint64_t n, uint64_t n_samples, uint32_t period) {
    return envelope_launch_ok(n_components, max_components, n_samples, period) && n % period == 0 && !((n / period) >> 32) && ranks.count != 0 &&
           ranks.count <= kQuantileMaxRanks && ranks.den != 0;
}
struct QuantileIndex { uint64_t lo, hi; };
// floor and ceiling of num * (m - 1) / den, m >= 1: num <= den < 2^32 and m <= 2^32, so the product stays below 2^64
SIXDOF_HOST_DEVICE inline QuantileIndex quantile_index(uint32_t num, uint32_t den, uint64_t m) {
    const uint64_t p = static_cast<uint64_t>(num) * (m - 1);
    const uint64_t lo = p / den;
    return {lo, lo + (p % den != 0 ? 1 : 0)};
}

// ---- the state of one (bin, rank) between passes --------------------------------------------------------------------------
constexpr uint32_t kQuantileEmpty = 1u;      // m == 0: nothing to select, the planes are NaN
constexpr uint32_t kQuantileNeedNext = 2u;   // x(hi) is the smallest key above x(lo): the closing min pass finds it
struct QuantileSlot {
    uint64_t prefix;   // the digits chosen so far, in place; after the last pass the key of x(lo)
    uint64_t k;        // the rank that is left: index of x(lo) among the elements that share the prefix
    uint64_t m;        // finite elements of the bin
    uint64_t lo, hi;
    uint32_t equal;    // elements in the digit chosen last; after the last pass: elements equal to x(lo)
    uint32_t flags;
};
SIXDOF_HOST_DEVICE inline uint64_t quantile_total(const uint32_t* hist) {
    uint64_t m = 0;
    for (uint32_t d = 0; d < kQuantileDigits; d++) m += hist[d];
    return m;
}
// The scan step: the digit whose counter holds rank k of the counted elements; k becomes the rank inside that digit.
SIXDOF_HOST_DEVICE inline uint32_t quantile_scan_step(const uint32_t* hist, uint64_t& k, uint32_t* in_digit) {
    uint32_t d = 0;
    for (; d + 1 < kQuantileDigits && k >= hist[d]; d++) k -= hist[d];
    *in_digit = hist[d];
    return d;
}
// The lo -> hi rule once `less` elements are below x(lo) and `equal` equal it: x(hi) == x(lo)?
SIXDOF_HOST_DEVICE inline bool quantile_hi_is_lo(uint64_t lo, uint64_t hi, uint64_t less, uint64_t equal) { return hi == lo || lo + 1 < less + equal; }
// Ranks of one bin whose prefixes are equal count the same elements: rank r reads the histogram of the first such rank.
SIXDOF_HOST_DEVICE inline uint32_t quantile_alias(const uint64_t* prefix, uint32_t r) {
    uint32_t a = 0;
    while (prefix[a] != prefix[r]) a++;
    return a;
}
// One (bin, rank) after pass `pass`, given the histogram of its alias.  Pass 0 also yields m, lo and hi.
SIXDOF_HOST_DEVICE inline void quantile_advance(QuantileSlot& s, const uint32_t* hist, uint32_t key_bits, uint32_t pass, uint32_t num, uint32_t den) {
    if (pass == 0) {
        s = QuantileSlot{};
        s.m = quantile_total(hist);
        if (s.m == 0) { s.flags = kQuantileEmpty; return; }
        const QuantileIndex i = quantile_index(num, den, s.m);
        s.lo = s.k = i.lo, s.hi = i.hi;
    }
    if (s.flags & kQuantileEmpty) return;
    const uint32_t d = quantile_scan_step(hist, s.k, &s.equal);
    s.prefix |= static_cast<uint64_t>(d) << quantile_shift(key_bits, pass);
    if (pass + 1 == quantile_passes(key_bits) && !quantile_hi_is_lo(s.lo, s.hi, s.lo - s.k, s.equal)) s.flags |= kQuantileNeedNext;
}
// The 1 + 2 * ranks planes of one bin are `plane_stride` apart; this writes rank r's two (and plane 0 with rank 0).
template <class E>
SIXDOF_HOST_DEVICE inline void quantile_emit(const QuantileSlot& s, uint64_t next_key, uint32_t r, double* out, uint64_t plane_stride) {
    const double nan = __builtin_nan("");
    const bool any = !(s.flags & kQuantileEmpty);
    if (r == 0) out[0] = static_cast<double>(s.m);
    const double lo = any ? QuantileBits<E>::value(s.prefix) : nan;
    out[(1 + 2 * r) * plane_stride] = lo;
    out[(2 + 2 * r) * plane_stride] = any && (s.flags & kQuantileNeedNext) ? QuantileBits<E>::value(next_key) : lo;
}

// ---- geometry: a pure function of (n, w, period, ranks) ----------------------------------------------------------------
struct QuantileGeom {
    uint32_t bins;         // period * w
    uint32_t cols;         // bins one block keeps: cols * ranks histograms in LDS
    uint32_t splits;       // column ranges: ceil(bins / cols)
    uint32_t sweep;        // rows a block reads at once: threads / cols
    uint32_t row_blocks;   // blocks that share the rows of one column range
    uint64_t rows;         // n / period
};
SIXDOF_HOST_DEVICE inline QuantileGeom quantile_geom(uint64_t n, uint32_t w, uint32_t period, uint32_t ranks) {
    QuantileGeom g{};
    g.bins = envelope_geom(n, w, period).bins;
    const uint32_t fit = kQuantileBlockSlots / ranks;
    g.cols = g.bins < fit ? g.bins : fit;
    g.splits = (g.bins + g.cols - 1) / g.cols;
    g.sweep = kQuantileThreads / g.cols;
    g.rows = n / period;
    const uint64_t sweeps = (g.rows + g.sweep - 1) / g.sweep;
    const uint64_t want = (sweeps + kQuantileSweepsPerBlock - 1) / kQuantileSweepsPerBlock;
    g.row_blocks = static_cast<uint32_t>(want < 1 ? 1 : want > kQuantileMaxRowBlocks ? kQuantileMaxRowBlocks : want);
    return g;
}

}  // namespace sixdof
