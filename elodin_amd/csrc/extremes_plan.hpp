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
// One tick of one component is a flat block of n * w elements; one thread owns element i and walks its samples in time order.
// The samples of a launch are cut into `segments` time segments (blockIdx.y); with more than one, every (segment, element)
// leaves a record in scratch and a merge launch folds them in time order.  The six output planes, [6][n * w] doubles per
// component, double as the accumulator a later call continues: extremes_emit and extremes_absorb are exact inverses.
#pragma once

#include <cstdint>

#include "quantile_plan.hpp"

namespace sixdof {

constexpr uint32_t kExtremesThreads = 256;         // threads of a block, one element each
constexpr uint32_t kExtremesPlanes = 6;            // SIXDOF_EXTREMES_PLANES: count, min, tick_min, max, tick_max, first_nonfinite
constexpr uint32_t kExtremesFields = 6;            // 64-bit fields of a record in scratch
constexpr uint32_t kExtremesLoads = 4;             // samples a thread loads before it uses the first
constexpr uint32_t kExtremesMaxSegments = 65535;   // the grid's y extent
constexpr uint64_t kExtremesMinChain = 16;         // no segment shorter than this by the plan's own choice
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
// Time segments of a read, a function of (n * w, n_samples) alone: n * w are the elements of the launch, all its components
// together.  A thread's samples form one chain of dependent compares but independent loads; what limits a small campaign is the
// number of waves, not the chain: 1,024 runs x 25 elements are 400 waves on 256 compute units.  So where the elements are fewer
// than kExtremesFillThreads (1,024 threads per compute unit) the samples are cut until that many threads run, no segment shorter
// than kExtremesMinChain samples; from there on one segment, which needs no scratch and no merge launch.  Chosen from the
// measured table in profiles/history_extremes.md: 1,024 ticks of 25,600 elements (1,024 bodies, the four Body columns) take
// 0.214 ms in one segment, 0.121 in 2, 0.076 in 4, 0.063 in 8, 0.057 in 16 and 0.064 in 32 — flat from 200,000 threads on; this
// rule picks 11 there (0.057 ms).  Sizes between that one and 65,536 bodies have not been measured.
SIXDOF_HOST_DEVICE inline uint32_t extremes_segments(uint64_t total, uint64_t n_samples) {
    if (total == 0 || total >= kExtremesFillThreads) return 1;
    uint64_t s = (kExtremesFillThreads + total - 1) / total;
    const uint64_t longest = n_samples / kExtremesMinChain;
    s = s > longest ? longest : s;
    s = s > kExtremesMaxSegments ? kExtremesMaxSegments : s;
    return static_cast<uint32_t>(s < 1 ? 1 : s);
}
// What a forced count (SIXDOF_EXTREMES_SEGMENTS) becomes: at least 1, at most one sample per segment and the grid's extent.
SIXDOF_HOST_DEVICE inline uint32_t extremes_clamp_segments(uint64_t forced, uint64_t n_samples) {
    uint64_t s = forced > n_samples ? n_samples : forced;
    s = s > kExtremesMaxSegments ? kExtremesMaxSegments : s;
    return static_cast<uint32_t>(s < 1 ? 1 : s);
}
// The most segments, at most `segments`, whose records of `units` elements fit `budget` bytes of scratch; 1 needs no scratch.
// Any count gives the same values: only time and memory depend on it.
SIXDOF_HOST_DEVICE inline uint32_t extremes_fit_segments(uint32_t segments, uint64_t units, uint64_t budget) {
    const uint64_t per_segment = units * kExtremesFields * sizeof(uint64_t);
    if (segments <= 1 || per_segment == 0) return segments < 1 ? 1 : segments;
    const uint64_t fit = budget / per_segment;
    return fit < 2 ? 1 : fit < segments ? static_cast<uint32_t>(fit) : segments;
}
SIXDOF_HOST_DEVICE inline uint64_t extremes_scratch_bytes(uint32_t segments, uint64_t units) {
    return segments <= 1 ? 0 : uint64_t(segments) * units * kExtremesFields * sizeof(uint64_t);
}
// Samples [lo, hi) of segment s: a balanced cut, every segment non-empty while segments <= n_samples.
SIXDOF_HOST_DEVICE inline uint64_t extremes_segment_start(uint64_t n_samples, uint32_t segments, uint32_t s) {
    return n_samples * s / segments;      // n_samples < 2^32 (the ring's size), s < 2^16
}

// Whether a double holds every sampled tick first_tick, first_tick + every, ...: the last one is below 2^53.  No step overflows.
inline bool extremes_ticks_ok(uint64_t first_tick, uint64_t n_samples, uint64_t every) {
    constexpr uint64_t limit = uint64_t(1) << 53;
    if (first_tick == 0 || first_tick >= limit || every == 0 || n_samples == 0) return false;
    return n_samples - 1 <= (limit - 1 - first_tick) / every;
}
// What launch_history_extremes accepts, for the launcher (extremes_kernels.hip) and its host twin (hip_fake.cpp) alike: at most
// `max_components` components, 1 .. n_samples segments within the grid's y extent, a sample count the segment cut can multiply,
// every component's elements within the grid's x extent, ticks that a double holds.
inline bool extremes_launch_ok(uint32_t n_components, uint32_t max_components, const uint32_t* widths, uint64_t n, uint64_t first_tick,
                               uint64_t n_samples, uint64_t every, uint32_t segments) {
    if (n_components == 0 || n_components > max_components || n_samples == 0 || (n_samples >> 32)) return false;
    if (segments == 0 || segments > kExtremesMaxSegments || segments > n_samples) return false;
    if (!extremes_ticks_ok(first_tick, n_samples, every)) return false;
    for (uint32_t k = 0; k < n_components; k++) {
        if (widths[k] == 0) return false;
        if (n != 0 && (n > ~uint64_t(0) / widths[k] || (n * widths[k] + kExtremesThreads - 1) / kExtremesThreads > 0x7fffffffull)) return false;
    }
    return true;
}

}  // namespace sixdof
