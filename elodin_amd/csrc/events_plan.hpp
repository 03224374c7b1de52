// events_plan.hpp — the record, the rule and the geometry of the ring events: per trigger and run, over the sampled ticks of a
// range, the first tick at which one element of one recorded component meets a threshold, and what the element held there and at
// the finite sample before.  Pure integer / compare code, no HIP: the kernels (events_kernels.hip) and the host twin
// (hip_fake.cpp) run the same functions — events_accumulate, events_merge, events_emit, events_tick_sampled — and nothing else for
// the rule, sixdof_history_events (sixdof_capi.cpp) sizes its buffers with the geometry below, events_host_test.cpp checks all of
// it on the host.
//
// A trigger reads element `element` of row run * period + group of every run (a run = `period` consecutive rows).  Its predicate
// is x op level, an IEEE compare of the ring's element widened to double (exact for f32) against a finite level, so -0.0 equals
// +0.0.  A non-finite sample is skipped as if it had not been sampled: it neither holds nor fails and is never a "before" sample.
// SIXDOF_EVENT_LEVEL: the earliest finite sample at which the predicate holds.  SIXDOF_EVENT_CROSSING: the earliest finite sample
// at which it holds and the previous finite sample did not — a predicate that holds from the first sample on never fires.
//
// The record does not know the mode.  It keeps the first finite sample, the last one and the first crossing; a LEVEL event is
// the first sample where that one holds, and the first crossing otherwise (events_emit).  Once a record has its crossing it is
// FROZEN: accumulate and merge leave it bit for bit.  The rule is exact and associative in time order, so the outputs cannot
// depend on how the samples of a range are cut into segments, launches or calls.  Ticks are counts of completed ticks (never 0
// for a sample, so 0 means "none").  One thread owns one (trigger, run) and walks its samples in time order: the walk (EventsRule
// below; the kernel writes scan_walk's loop out), the cut into time segments and the scratch of their records are time_scan.hpp's.
#pragma once

#include <cstdint>

#include "quantile_plan.hpp"
#include "time_scan.hpp"

namespace sixdof {

constexpr uint32_t kEventsThreads = 256;         // threads of a block
constexpr uint32_t kEventsPlanes = 4;            // SIXDOF_EVENTS_PLANES: tick, value, tick before, value before
constexpr uint32_t kEventsFields = 10;           // 64-bit fields of a record
constexpr uint32_t kEventsMaxTriggers = 8;       // SIXDOF_EVENTS_MAX_TRIGGERS
constexpr uint64_t kEventsFillThreads = 16384;   // threads below which the plan cuts the samples: see events_segments

constexpr uint32_t kEventLt = 0, kEventLe = 1, kEventGt = 2, kEventGe = 3;   // SIXDOF_EVENT_LT ..
constexpr uint32_t kEventLevel = 0, kEventCrossing = 1;                      // SIXDOF_EVENT_LEVEL, SIXDOF_EVENT_CROSSING

struct EventsRecord {
    uint64_t first_tick, first_bits, first_holds;      // the first finite sample (tick 0: none yet): raw bits, predicate 0 / 1
    uint64_t last_tick, last_bits, last_holds;         // the last finite sample before the crossing, or of all
    uint64_t event_tick, event_bits;                   // the first crossing (tick 0: none yet)
    uint64_t before_tick, before_bits;                 // the finite sample before it
};
SIXDOF_HOST_DEVICE inline EventsRecord events_empty() { return {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; }

// One sample, later than every sample `rec` has met.
SIXDOF_HOST_DEVICE inline void events_accumulate(EventsRecord& rec, uint64_t bits, uint64_t tick, bool finite, bool holds) {
    // selects per field, not branches over groups of fields: the record stays in registers on the device
    const bool live = finite && rec.event_tick == 0;                                   // not skipped, not frozen
    const bool first = live && rec.first_tick == 0;
    const bool cross = live && !first && holds && rec.last_holds == 0;
    const bool last = live && !cross;                                                  // the crossing itself is no "last" sample
    rec.first_tick = first ? tick : rec.first_tick, rec.first_bits = first ? bits : rec.first_bits, rec.first_holds = first ? uint64_t(holds) : rec.first_holds;
    rec.event_tick = cross ? tick : rec.event_tick, rec.event_bits = cross ? bits : rec.event_bits;
    rec.before_tick = cross ? rec.last_tick : rec.before_tick, rec.before_bits = cross ? rec.last_bits : rec.before_bits;
    rec.last_tick = last ? tick : rec.last_tick, rec.last_bits = last ? bits : rec.last_bits, rec.last_holds = last ? uint64_t(holds) : rec.last_holds;
}
// `later` holds samples that all come after those of `earlier`.
SIXDOF_HOST_DEVICE inline EventsRecord events_merge(const EventsRecord& earlier, const EventsRecord& later) {
    if (earlier.event_tick != 0 || later.first_tick == 0) return earlier;   // frozen, or nothing to add
    if (earlier.first_tick == 0) return later;
    EventsRecord r = earlier;
    if (later.first_holds && !earlier.last_holds) {   // the crossing spans the cut: it falls on `later`'s first finite sample
        r.event_tick = later.first_tick, r.event_bits = later.first_bits, r.before_tick = earlier.last_tick, r.before_bits = earlier.last_bits;
        return r;
    }
    r.last_tick = later.last_tick, r.last_bits = later.last_bits, r.last_holds = later.last_holds;
    r.event_tick = later.event_tick, r.event_bits = later.event_bits, r.before_tick = later.before_tick, r.before_bits = later.before_bits;
    return r;
}
// Nothing a later sample could add changes what `mode` reports: the record is frozen, or its first sample is the LEVEL event
// (the first sample of a merged record is the earlier one's).  A walk may stop there.
SIXDOF_HOST_DEVICE inline bool events_settled(const EventsRecord& r, uint32_t mode) {
    return r.event_tick != 0 || (mode == kEventLevel && r.first_tick != 0 && r.first_holds != 0);
}
// The tick `mode` reports, from the three fields that decide it; 0: none.
SIXDOF_HOST_DEVICE inline uint64_t events_tick(uint64_t first_tick, uint64_t first_holds, uint64_t event_tick, uint32_t mode) {
    return mode == kEventLevel && first_tick != 0 && first_holds != 0 ? first_tick : event_tick;
}

// The ring's element as the predicate and the outputs see it: raw bits, widened to double (exact for f32).
template <class E>
SIXDOF_HOST_DEVICE inline double events_value(uint64_t bits) {
    if (sizeof(E) == 8) { double x; __builtin_memcpy(&x, &bits, 8); return x; }
    const uint32_t u = static_cast<uint32_t>(bits);
    float f;
    __builtin_memcpy(&f, &u, 4);
    return static_cast<double>(f);
}
SIXDOF_HOST_DEVICE inline bool events_holds(double x, uint32_t op, double level) {
    return op == kEventLt ? x < level : op == kEventLe ? x <= level : op == kEventGt ? x > level : x >= level;
}
// One trigger element's sample: the rule applied to what the ring holds.
template <class E>
SIXDOF_HOST_DEVICE inline void events_sample(EventsRecord& rec, E x, uint64_t tick, uint32_t op, double level) {
    const uint64_t u = QuantileBits<E>::raw(x);
    events_accumulate(rec, u, tick, QuantileBits<E>::finite(u), events_holds(static_cast<double>(x), op, level));
}
// The rule of one trigger as scan_walk takes it: a walk ends where its record is settled.
struct EventsRule {
    double level;
    uint32_t op, mode;
    template <class E>
    SIXDOF_HOST_DEVICE void sample(EventsRecord& rec, E x, uint64_t tick) const { events_sample<E>(rec, x, tick, op, level); }
    SIXDOF_HOST_DEVICE bool settled(const EventsRecord& rec) const { return events_settled(rec, mode); }
};

// The four planes of one (trigger, run), `plane_stride` doubles apart: event tick (0: none), the value at it (NaN: none), the
// tick of the finite sample before it (0: none) and that sample's value (NaN: none).  Conversions only.
template <class E>
SIXDOF_HOST_DEVICE inline void events_emit(const EventsRecord& r, uint32_t mode, double* out, uint64_t plane_stride) {
    const double nan = __builtin_nan("");
    const bool at_first = mode == kEventLevel && r.first_tick != 0 && r.first_holds != 0;
    const bool crossed = !at_first && r.event_tick != 0;
    out[0] = static_cast<double>(at_first ? r.first_tick : r.event_tick);
    out[plane_stride] = at_first ? events_value<E>(r.first_bits) : crossed ? events_value<E>(r.event_bits) : nan;
    out[2 * plane_stride] = crossed ? static_cast<double>(r.before_tick) : 0.0;
    out[3 * plane_stride] = crossed ? events_value<E>(r.before_bits) : nan;
}

// A record in a record buffer or in scratch: field f of unit u at base[f * stride + u], so that consecutive lanes store
// consecutive words.
SIXDOF_HOST_DEVICE inline void events_store(const EventsRecord& r, uint64_t* base, uint64_t stride) {
    base[0] = r.first_tick, base[stride] = r.first_bits, base[2 * stride] = r.first_holds;
    base[3 * stride] = r.last_tick, base[4 * stride] = r.last_bits, base[5 * stride] = r.last_holds;
    base[6 * stride] = r.event_tick, base[7 * stride] = r.event_bits, base[8 * stride] = r.before_tick, base[9 * stride] = r.before_bits;
}
SIXDOF_HOST_DEVICE inline EventsRecord events_load(const uint64_t* base, uint64_t stride) {
    return {base[0],          base[stride],     base[2 * stride], base[3 * stride], base[4 * stride],
            base[5 * stride], base[6 * stride], base[7 * stride], base[8 * stride], base[9 * stride]};
}
// The tick `mode` reports, out of a stored record.
SIXDOF_HOST_DEVICE inline uint64_t events_stored_tick(const uint64_t* base, uint64_t stride, uint32_t mode) {
    return events_tick(base[0], base[2 * stride], base[6 * stride], mode);
}

// Whether `tick` is one of the call's samples first_tick, first_tick + every, ..., `last`; only then may a slot be formed of it.
SIXDOF_HOST_DEVICE inline bool events_tick_sampled(uint64_t tick, uint64_t first_tick, uint64_t last, uint64_t every) {
    return tick >= first_tick && tick <= last && (tick - first_tick) % every == 0;
}

// ---- geometry -------------------------------------------------------------------------------------------------------------
// Time segments of a read, scan_segments of (runs x triggers, n_samples).  The extremes' threshold (262,144 threads) was measured
// for a walk whose lanes read consecutive elements, not for this one, whose lanes are period * w elements apart — a wave's load
// touches w times the cache lines — and whose settled threads stop early.  The threshold here is chosen from the forced-segment
// table in profiles/history_events.md (one world_pos trigger, 1,024 ticks): at 1,024 runs 0.315 ms in one segment, 0.170 in 2,
// 0.098 in 4, 0.064 in 8, 0.052 in 16, 0.055 in 32 and 0.079 in 64; at 65,536 runs 0.626 ms in one, 0.638 in 2, 0.655 in 4 and
// 0.70 from 8 on.  So about 16,384 threads fill the chip for this walk: the rule picks 16 at 1,024 runs and 1 at 65,536.  Sizes
// between the two, and the chain length, have not been measured.
SIXDOF_HOST_DEVICE inline uint32_t events_segments(uint64_t units, uint64_t n_samples) { return scan_segments(units, n_samples, kEventsFillThreads); }
// The record buffer of `units` (trigger, run) pairs: what a continuing call starts from.
SIXDOF_HOST_DEVICE inline uint64_t events_record_bytes(uint64_t units) { return units * kEventsFields * sizeof(uint64_t); }

// One trigger as the kernels see it.
struct EventsTrigger {
    const void* ring;    // [ring][n, w] blocks of its component
    double level;
    uint32_t w, element, group, op, mode, reserved;
};
struct EventsArgs { EventsTrigger t[kEventsMaxTriggers]; };   // by value: 320 bytes of kernel arguments

// What launch_history_events accepts, for the launcher (events_kernels.hip) and its host twin (hip_fake.cpp) alike: 1 to 8
// triggers that name an element of their component, a row of a run, an op and a mode and hold a finite level; whole runs, within
// the grid's x extent; 1 .. n_samples segments within the grid's y extent; ticks that a double holds.
inline bool events_launch_ok(const EventsArgs& a, uint32_t n_triggers, uint64_t n, uint32_t period, uint64_t first_tick, uint64_t n_samples,
                             uint64_t every, uint32_t segments) {
    if (n_triggers == 0 || n_triggers > kEventsMaxTriggers || period == 0 || n % period != 0) return false;
    if (n_samples == 0 || (n_samples >> 32) || segments == 0 || segments > kScanMaxSegments || segments > n_samples) return false;
    if (!scan_ticks_ok(first_tick, n_samples, every)) return false;
    if ((n / period + kEventsThreads - 1) / kEventsThreads > 0x7fffffffull) return false;
    for (uint32_t k = 0; k < n_triggers; k++) {
        const EventsTrigger& t = a.t[k];
        if (t.w == 0 || t.element >= t.w || t.group >= period || t.op > kEventGe || t.mode > kEventCrossing) return false;
        if (!QuantileBits<double>::finite(QuantileBits<double>::raw(t.level))) return false;
        if (n != 0 && n > ~uint64_t(0) / t.w) return false;
    }
    return true;
}
// What launch_events_capture accepts: 1 to `max_components` captured components, every one's elements within the grid's x extent.
inline bool events_capture_ok(const EventsArgs& a, uint32_t n_triggers, uint32_t n_captures, uint32_t max_components, const uint32_t* widths, uint64_t n,
                              uint32_t period, uint64_t first_tick, uint64_t n_samples, uint64_t every) {
    if (n_captures == 0 || n_captures > max_components) return false;
    if (!events_launch_ok(a, n_triggers, n, period, first_tick, n_samples, every, 1)) return false;
    for (uint32_t k = 0; k < n_captures; k++) {
        if (widths[k] == 0) return false;
        if (n != 0 && (n > ~uint64_t(0) / widths[k] || (n * widths[k] + kEventsThreads - 1) / kEventsThreads > 0x7fffffffull)) return false;
    }
    return true;
}

}  // namespace sixdof
