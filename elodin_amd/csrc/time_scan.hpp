// time_scan.hpp — what the readers that collapse the ring ACROSS TIME share: the ring extremes (extremes_plan.hpp) and the ring
// events (events_plan.hpp).  Pure integer arithmetic and one loop, no HIP: extremes_walk_kernel (extremes_kernels.hip) and both
// host twins (hip_fake.cpp) run the same scan_walk — events_walk_kernel (events_kernels.hip) has the same loop written out, for the
// one per cent it measured —, sixdof_capi.cpp's time_scan_read sizes scratch with the geometry, extremes_host_test.cpp and
// events_host_test.cpp check all of it on the host.
//
// A scan has a record and a rule that is exact and associative in time order.  One thread per unit (an element, a run) walks the
// samples of a range in time order; the samples of a launch are cut into `segments` time segments (blockIdx.y).  With more than
// one, every (segment, unit) leaves its record in scratch, `fields` 64-bit words each, and a merge launch folds them in time
// order — so no result can depend on the cut.  What a reader adds: its record, its rule (sample, settled, merge), how a record
// is stored, loaded and turned into output planes, and the thread count that fills the chip for its walk.
#pragma once

#include <cstdint>

#include "history_plan.hpp"

namespace sixdof {

constexpr uint32_t kScanLoads = 4;             // samples a thread loads before it uses the first
constexpr uint32_t kScanMaxSegments = 65535;   // the grid's y extent
constexpr uint64_t kScanMinChain = 16;         // no segment shorter than this by a plan's own choice

// ---- geometry -------------------------------------------------------------------------------------------------------------
// Time segments of a launch, a function of (units, n_samples) and the reader's `fill_threads` alone.  A thread's samples form
// one chain of dependent compares but independent loads; what limits a small campaign is the number of waves, not the chain.  So
// where the units are fewer than fill_threads the samples are cut until that many threads run, no segment shorter than
// kScanMinChain samples; from there on one segment, which needs no scratch and no merge launch.
SIXDOF_HOST_DEVICE inline uint32_t scan_segments(uint64_t units, uint64_t n_samples, uint64_t fill_threads) {
    if (units == 0 || units >= fill_threads) return 1;
    uint64_t s = (fill_threads + units - 1) / units;
    const uint64_t longest = n_samples / kScanMinChain;
    s = s > longest ? longest : s;
    s = s > kScanMaxSegments ? kScanMaxSegments : s;
    return static_cast<uint32_t>(s < 1 ? 1 : s);
}
// What a forced count (SIXDOF_EXTREMES_SEGMENTS, SIXDOF_EVENTS_SEGMENTS) becomes: at least 1, at most one sample per segment and
// the grid's extent.
SIXDOF_HOST_DEVICE inline uint32_t scan_clamp_segments(uint64_t forced, uint64_t n_samples) {
    uint64_t s = forced > n_samples ? n_samples : forced;
    s = s > kScanMaxSegments ? kScanMaxSegments : s;
    return static_cast<uint32_t>(s < 1 ? 1 : s);
}
// The most segments, at most `segments`, whose records of `units` units x `fields` words fit `budget` bytes of scratch; 1 needs
// no scratch.  Any count gives the same values: only time and memory depend on it.
SIXDOF_HOST_DEVICE inline uint32_t scan_fit_segments(uint32_t segments, uint64_t units, uint32_t fields, uint64_t budget) {
    const uint64_t per_segment = units * fields * sizeof(uint64_t);
    if (segments <= 1 || per_segment == 0) return segments < 1 ? 1 : segments;
    const uint64_t fit = budget / per_segment;
    return fit < 2 ? 1 : fit < segments ? static_cast<uint32_t>(fit) : segments;
}
SIXDOF_HOST_DEVICE inline uint64_t scan_scratch_bytes(uint32_t segments, uint64_t units, uint32_t fields) {
    return segments <= 1 ? 0 : uint64_t(segments) * units * fields * sizeof(uint64_t);
}
// Samples [lo, hi) of segment s: a balanced cut, every segment non-empty while segments <= n_samples.
SIXDOF_HOST_DEVICE inline uint64_t scan_segment_start(uint64_t n_samples, uint32_t segments, uint32_t s) {
    return n_samples * s / segments;      // n_samples < 2^32 (the ring's size), s < 2^16
}
// Whether a double holds every sampled tick first_tick, first_tick + every, ...: the last one is below 2^53.  No step overflows.
SIXDOF_HOST_DEVICE inline bool scan_ticks_ok(uint64_t first_tick, uint64_t n_samples, uint64_t every) {
    constexpr uint64_t limit = uint64_t(1) << 53;
    if (first_tick == 0 || first_tick >= limit || every == 0 || n_samples == 0) return false;
    return n_samples - 1 <= (limit - 1 - first_tick) / every;
}

// ---- the walk -------------------------------------------------------------------------------------------------------------
// The record `r` after samples [lo, hi) of the range, in time order: sample j is src[slot(j) * stride] at tick
// first_tick + j * every.  The addresses of a unit's samples do not depend on each other: kScanLoads of them are loaded before the
// first is used, and the slot advances by an add and a compare, not a division.  rule.sample(r, x, tick) applies one sample; once
// rule.settled(r) says that no later sample can change what the reader reports, the walk stops loading.  Record and rule travel by
// value: a record behind a reference cost the extremes' walk six registers and 2 to 5 % of its time
// (profiles/time_scan_refactor.md).
template <class E, class Record, class Rule>
SIXDOF_HOST_DEVICE inline Record scan_walk(Record r, const Rule rule, const E* __restrict__ src, uint64_t stride, uint64_t lo, uint64_t hi,
                                           uint64_t first_tick, uint64_t every, uint64_t ring) {
    const uint64_t step = every % ring;
    uint64_t slot = sample_slot(first_tick, lo, every, ring), tick = first_tick + lo * every;
    uint64_t j = lo;
    for (; j + kScanLoads <= hi && !rule.settled(r); j += kScanLoads) {
        E x[kScanLoads];
#pragma unroll
        for (uint32_t q = 0; q < kScanLoads; q++) {
            x[q] = src[slot * stride];
            slot = next_sample_slot(slot, step, ring);
        }
#pragma unroll
        for (uint32_t q = 0; q < kScanLoads; q++) {
            rule.sample(r, x[q], tick);
            tick += every;
        }
    }
    for (; j < hi && !rule.settled(r); j++) {
        rule.sample(r, src[slot * stride], tick);
        slot = next_sample_slot(slot, step, ring);
        tick += every;
    }
    return r;
}

}  // namespace sixdof
