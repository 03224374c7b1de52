// norm_events_plan.hpp — the ring norm events: per trigger and run, over the sampled ticks of a range, the first tick at which a
// SQUARED Euclidean norm — of 1 to 4 consecutive elements of one row, or of their difference to as many elements of another row
// of the same run — meets a squared level, and what the norm held there and at the finite sample before.  Nothing here is new
// arithmetic: the value is norms_plan.hpp's norms_value (f64, left to right, no FMA contraction), the walk its norms_walk_with
// (norms_depth samples loaded before the first value is formed), the record and the rule events_plan.hpp's events_accumulate,
// events_merge, events_settled and events_emit<double>, the cut into time segments time_scan.hpp's.  This header joins them: the
// rule that hands a squared norm to the events' record (NormEventsRule), the arguments, the geometry and the launch check.  The
// kernels (norm_events_kernels.hip) and the host twin (hip_fake.cpp) run the same functions, sixdof_history_norm_events
// (sixdof_capi.cpp) sizes its buffers with the geometry below, norm_events_host_test.cpp checks all of it on the host.
//
// A sample is finite exactly when s is: an overflowing square is skipped like any non-finite sample — it neither holds nor fails
// and is never a "before" sample.  The predicate is the IEEE compare s op level_sq: no square root, no other arithmetic.  The
// record keeps the raw bits of the double s on either handle type, so the planes come from events_emit<double>.
#pragma once

#include <cstdint>

#include "events_plan.hpp"
#include "norms_plan.hpp"

namespace sixdof {

constexpr uint32_t kNormEventsThreads = 256;                    // threads of a block, one run each
constexpr uint32_t kNormEventsPlanes = kEventsPlanes;           // SIXDOF_NORM_EVENTS_PLANES: tick, s, tick before, s before
constexpr uint32_t kNormEventsFields = kEventsFields;           // 64-bit fields of a record
constexpr uint32_t kNormEventsMaxTriggers = kEventsMaxTriggers; // SIXDOF_NORM_EVENTS_MAX_TRIGGERS
// Threads below which the plan cuts the samples (norm_events_segments).  Not derivable: it started from the parents' 16,384 (the
// events' and the norms' walks, whose lanes are period * w elements apart as here), and the forced-segment table of
// profiles/history_norm_events.md (one never-firing |v| trigger, 1,024 ticks, reduced only, one MI355X) confirms that value for
// this walk: at 1,024 runs 0.316 ms in one segment, 0.170 in 2, 0.097 in 4, 0.063 in 8, 0.051 in 16 and 0.057 in 32; at 65,536
// runs 1.031 ms in one, 1.056 in 2, 1.064 in 4 and 1.10 from 8 on.  So the rule picks 16 at 1,024 runs (the table's minimum) and 1
// at 65,536.  Sizes between the two, and the chain length, have not been measured.
constexpr uint64_t kNormEventsFillThreads = 16384;

// One trigger as the kernels see it: the probe of norms_plan.hpp and the predicate s op level_sq.
struct NormEventsTrigger {
    NormsProbe probe;
    double level_sq;      // finite, >= 0
    uint32_t op, mode;    // kEventLt .. kEventGe; kEventLevel, kEventCrossing
};
struct NormEventsArgs { NormEventsTrigger t[kNormEventsMaxTriggers]; };   // by value: 512 bytes of kernel arguments
static_assert(sizeof(NormEventsTrigger) == 64 && sizeof(NormEventsArgs) == 512, "NormEventsArgs is 8 x 64 bytes");

// One squared norm, later than every sample `rec` has met: the events' rule applied to the derived scalar, bits unchanged.
SIXDOF_HOST_DEVICE inline void norm_events_sample(EventsRecord& rec, double s, uint64_t tick, uint32_t op, double level_sq) {
    const uint64_t u = QuantileBits<double>::raw(s);
    events_accumulate(rec, u, tick, QuantileBits<double>::finite(u), events_holds(s, op, level_sq));
}
// The rule of one trigger as norms_walk_as takes it: a walk ends where its record is settled.
struct NormEventsRule {
    double level_sq;
    uint32_t op, mode;
    SIXDOF_HOST_DEVICE void sample(EventsRecord& rec, double s, uint64_t tick) const { norm_events_sample(rec, s, tick, op, level_sq); }
    SIXDOF_HOST_DEVICE bool settled(const EventsRecord& rec) const { return events_settled(rec, mode); }
};
// The record `r` (the accumulator's on a continuing one-segment launch, else empty) after samples [lo, hi) of trigger `t` for run
// `run`: what the kernel and the host twin both call.
template <class E>
SIXDOF_HOST_DEVICE inline EventsRecord norm_events_walk(EventsRecord r, const NormEventsTrigger& t, uint64_t run, uint64_t n, uint32_t period, uint64_t lo,
                                                        uint64_t hi, uint64_t first_tick, uint64_t every, uint64_t ring) {
    return norms_walk_with<E>(r, NormEventsRule{t.level_sq, t.op, t.mode}, t.probe, run, n, period, lo, hi, first_tick, every, ring);
}

// Where the record of (trigger, run) sits in the record buffer and that of (segment, trigger, run) in scratch — field f at
// base[f * runs], so that consecutive lanes store consecutive words — and where the four planes of (trigger, run) sit in the
// output, `runs` doubles apart.  The record buffer's layout is the events': launch_events_capture reads it.
SIXDOF_HOST_DEVICE inline uint64_t norm_events_record_index(uint32_t trig, uint64_t runs, uint64_t run) { return uint64_t(trig) * kNormEventsFields * runs + run; }
SIXDOF_HOST_DEVICE inline uint64_t norm_events_scratch_index(uint32_t seg, uint32_t n_triggers, uint32_t trig, uint64_t runs, uint64_t run) {
    return (uint64_t(seg) * n_triggers + trig) * kNormEventsFields * runs + run;
}
SIXDOF_HOST_DEVICE inline uint64_t norm_events_out_index(uint32_t trig, uint64_t runs, uint64_t run) { return uint64_t(trig) * kNormEventsPlanes * runs + run; }

// ---- geometry -------------------------------------------------------------------------------------------------------------
// Time segments of a read, scan_segments of (runs x triggers, n_samples) under kNormEventsFillThreads.
SIXDOF_HOST_DEVICE inline uint32_t norm_events_segments(uint64_t units, uint64_t n_samples) { return scan_segments(units, n_samples, kNormEventsFillThreads); }

// The EventsArgs that launch_events_capture is handed for these triggers: it reads each trigger's mode, and its check
// (events_capture_ok) wants an element of a row of a run, an op, a mode and a finite level — the probe's first element, its
// group, the trigger's op, mode and level_sq are such.  The capture reads neither ring nor level.
inline EventsArgs norm_events_capture_args(const NormEventsArgs& a, uint32_t n_triggers) {
    EventsArgs e{};
    for (uint32_t k = 0; k < n_triggers && k < kNormEventsMaxTriggers; k++) {
        const NormEventsTrigger& t = a.t[k];
        e.t[k] = {t.probe.ring_a, t.level_sq, t.probe.w_a, t.probe.element_a, t.probe.group_a, t.op, t.mode, 0};
    }
    return e;
}

// What launch_history_norm_events accepts, for the launcher (norm_events_kernels.hip) and its host twin (hip_fake.cpp) alike:
// what norms_launch_ok asks of the probes and the range, what events_launch_ok asks of op and mode, and a squared level that is
// finite and not below 0 (-0.0 is not below 0).
inline bool norm_events_launch_ok(const NormEventsArgs& a, uint32_t n_triggers, uint64_t n, uint32_t period, uint64_t first_tick, uint64_t n_samples,
                                  uint64_t every, uint32_t segments) {
    if (n_triggers == 0 || n_triggers > kNormEventsMaxTriggers) return false;
    NormsArgs probes{};
    for (uint32_t k = 0; k < n_triggers; k++) {
        const NormEventsTrigger& t = a.t[k];
        if (t.op > kEventGe || t.mode > kEventCrossing) return false;
        if (!QuantileBits<double>::finite(QuantileBits<double>::raw(t.level_sq)) || t.level_sq < 0.0) return false;
        probes.p[k] = t.probe;
    }
    static_assert(kNormEventsMaxTriggers == kNormsMaxProbes && kNormEventsThreads == kNormsThreads, "the probes are checked by norms_launch_ok");
    return norms_launch_ok(probes, n_triggers, n, period, first_tick, n_samples, every, segments);
}

}  // namespace sixdof
