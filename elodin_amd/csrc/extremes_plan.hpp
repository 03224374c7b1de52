// extremes_plan.hpp — the record, the rule and the geometry of the ring extremes: per row and component element, over the sampled
// ticks of a range, the count of finite samples, the smallest and the largest finite value with the EARLIEST sampled tick that
// holds each, and the earliest sampled tick at which the element is not finite.  Pure integer arithmetic, no HIP: the kernels
// (extremes_kernels.hip) and the host twin (hip_fake.cpp) run the same two functions — extremes_accumulate and extremes_merge
// — and nothing else for the rule, sixdof_history_extremes (sixdof_capi.cpp) sizes its scratch with the geometry below,
// extremes_host_test.cpp checks all of it on the host.
//
// Values are compared as quantile_plan.hpp's order-preserving integer keys (-0.0 below +0.0), ticks are counts of completed
// ticks (never 0 for a sample, so 0 means "none").  The rule is exact and associative in time order: a later sample replaces an
// extreme only when its key is STRICTLY smaller or larger, the earlier non-finite tick wins.  So the result cannot depend on how
// the samples of a range are cut into segments, launches or calls.
//
// One tick of one component is a flat block of n * w elements; one thread owns element i and walks its samples in time order:
// the walk, the cut into time segments and the scratch of their records are time_scan.hpp's.  The six output planes,
// [6][n * w] doubles per component, double as the accumulator a later call continues: extremes_emit and extremes_absorb are
// exact inverses.
#pragma once

#include <cstdint>

#include "quantile_plan.hpp"
#include "time_scan.hpp"

namespace sixdof {

constexpr uint32_t kExtremesThreads = 256;         // threads of a block, one element each
constexpr uint32_t kExtremesPlanes = 6;            // SIXDOF_EXTREMES_PLANES: count, min, tick_min, max, tick_max, first_nonfinite
constexpr uint32_t kExtremesFields = 6;            // 64-bit fields of a record in scratch
constexpr uint64_t kExtremesFillThreads = 262144;  // threads below which the plan cuts the samples: see extremes_segments

// The identity: no finite key is ~0 (a positive NaN pattern) or 0 (a negative one), so the strict comparisons of the rule need
// no look at `count`.
struct ExtremesRecord {
    uint64_t count;             // samples at which the element is finite
    uint64_t key_min, tick_min;
    uint64_t key_max, tick_max;
    uint64_t first_nonfinite;   // 0: none
};
SIXDOF_HOST_DEVICE inline ExtremesRecord extremes_empty() { return {0, ~uint64_t(0), 0, 0, 0, 0}; }

// One sample, later than every sample `rec` has met.
SIXDOF_HOST_DEVICE inline void extremes_accumulate(ExtremesRecord& rec, uint64_t key, uint64_t tick, bool finite) {
    if (!finite) {
        rec.first_nonfinite = rec.first_nonfinite ? rec.first_nonfinite : tick;
        return;
    }
    rec.count++;
    if (key < rec.key_min) rec.key_min = key, rec.tick_min = tick;
    if (key > rec.key_max) rec.key_max = key, rec.tick_max = tick;
}
// `later` holds samples that all come after those of `earlier`.
SIXDOF_HOST_DEVICE inline ExtremesRecord extremes_merge(const ExtremesRecord& earlier, const ExtremesRecord& later) {
    ExtremesRecord r = earlier;
    r.count += later.count;
    if (later.key_min < r.key_min) r.key_min = later.key_min, r.tick_min = later.tick_min;
    if (later.key_max > r.key_max) r.key_max = later.key_max, r.tick_max = later.tick_max;
    r.first_nonfinite = r.first_nonfinite ? r.first_nonfinite : later.first_nonfinite;
    return r;
}
// One element's sample: the rule applied to what the ring holds.
template <class E>
SIXDOF_HOST_DEVICE inline void extremes_sample(ExtremesRecord& rec, E x, uint64_t tick) {
    const uint64_t u = QuantileBits<E>::raw(x);
    extremes_accumulate(rec, QuantileBits<E>::key(u), tick, QuantileBits<E>::finite(u));
}
// The rule as scan_walk takes it: every sample counts, so no walk ends early.
struct ExtremesRule {
    template <class E>
    SIXDOF_HOST_DEVICE void sample(ExtremesRecord& rec, E x, uint64_t tick) const { extremes_sample<E>(rec, x, tick); }
    SIXDOF_HOST_DEVICE bool settled(const ExtremesRecord&) const { return false; }
};

// The six planes of one element, `plane_stride` doubles apart.  Conversions only: a key back to its value (f32 widened, which is
// exact), an integer below 2^53 to the double that holds it.
template <class E>
SIXDOF_HOST_DEVICE inline void extremes_emit(const ExtremesRecord& r, double* out, uint64_t plane_stride) {
    const double nan = __builtin_nan("");
    const bool any = r.count != 0;
    out[0] = static_cast<double>(r.count);
    out[plane_stride] = any ? QuantileBits<E>::value(r.key_min) : nan;
    out[2 * plane_stride] = static_cast<double>(r.tick_min);
    out[3 * plane_stride] = any ? QuantileBits<E>::value(r.key_max) : nan;
    out[4 * plane_stride] = static_cast<double>(r.tick_max);
    out[5 * plane_stride] = static_cast<double>(r.first_nonfinite);
}
// The record those planes came from: what a continuing call merges into.
template <class E>
SIXDOF_HOST_DEVICE inline ExtremesRecord extremes_absorb(const double* out, uint64_t plane_stride) {
    ExtremesRecord r = extremes_empty();
    r.count = static_cast<uint64_t>(out[0]);
    if (r.count != 0) {
        r.key_min = QuantileBits<E>::key(QuantileBits<E>::raw(static_cast<E>(out[plane_stride])));
        r.tick_min = static_cast<uint64_t>(out[2 * plane_stride]);
        r.key_max = QuantileBits<E>::key(QuantileBits<E>::raw(static_cast<E>(out[3 * plane_stride])));
        r.tick_max = static_cast<uint64_t>(out[4 * plane_stride]);
    }
    r.first_nonfinite = static_cast<uint64_t>(out[5 * plane_stride]);
    return r;
}

// A record in scratch: field f of unit u at base[f * stride + u], so that consecutive lanes store consecutive words.
SIXDOF_HOST_DEVICE inline void extremes_store(const ExtremesRecord& r, uint64_t* base, uint64_t stride) {
    base[0] = r.count, base[stride] = r.key_min, base[2 * stride] = r.tick_min;
    base[3 * stride] = r.key_max, base[4 * stride] = r.tick_max, base[5 * stride] = r.first_nonfinite;
}
SIXDOF_HOST_DEVICE inline ExtremesRecord extremes_load(const uint64_t* base, uint64_t stride) {
    return {base[0], base[stride], base[2 * stride], base[3 * stride], base[4 * stride], base[5 * stride]};
}

// ---- geometry -------------------------------------------------------------------------------------------------------------
// Time segments of a read, scan_segments of (n * w, n_samples): n * w are the elements of the launch, all its components
// together.  What limits a small campaign is the number of waves: 1,024 runs x 25 elements are 400 waves on 256 compute units.
// So the samples are cut where the elements are fewer than kExtremesFillThreads (1,024 threads per compute unit).  Chosen from
// the measured table in profiles/history_extremes.md: 1,024 ticks of 25,600 elements (1,024 bodies, the four Body columns) take
// 0.214 ms in one segment, 0.121 in 2, 0.076 in 4, 0.063 in 8, 0.057 in 16 and 0.064 in 32 — flat from 200,000 threads on; this
// rule picks 11 there (0.057 ms).  Sizes between that one and 65,536 bodies have not been measured.
SIXDOF_HOST_DEVICE inline uint32_t extremes_segments(uint64_t total, uint64_t n_samples) { return scan_segments(total, n_samples, kExtremesFillThreads); }

// What launch_history_extremes accepts, for the launcher (extremes_kernels.hip) and its host twin (hip_fake.cpp) alike: at most
// `max_components` components, 1 .. n_samples segments within the grid's y extent, a sample count the segment cut can multiply,
// every component's elements within the grid's x extent, ticks that a double holds.
inline bool extremes_launch_ok(uint32_t n_components, uint32_t max_components, const uint32_t* widths, uint64_t n, uint64_t first_tick,
                               uint64_t n_samples, uint64_t every, uint32_t segments) {
    if (n_components == 0 || n_components > max_components || n_samples == 0 || (n_samples >> 32)) return false;
    if (segments == 0 || segments > kScanMaxSegments || segments > n_samples) return false;
    if (!scan_ticks_ok(first_tick, n_samples, every)) return false;
    for (uint32_t k = 0; k < n_components; k++) {
        if (widths[k] == 0) return false;
        if (n != 0 && (n > ~uint64_t(0) / widths[k] || (n * widths[k] + kExtremesThreads - 1) / kExtremesThreads > 0x7fffffffull)) return false;
    }
    return true;
}

}  // namespace sixdof
