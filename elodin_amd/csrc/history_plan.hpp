// history_plan.hpp — where a recorded tick sits in the telemetry ring, and which sampled ranges can be read from it.  Pure
// arithmetic, no HIP.  Every reader of the ring validates with it — sixdof_history_read, sixdof_history_stream,
// sixdof_watch_read, sixdof_history_envelope, sixdof_history_quantiles, sixdof_history_extremes, sixdof_history_events (sixdof_capi.cpp) — and everything that touches a slot
// addresses with it: those readers, snapshot_tick_to_ring and sixdof_step's overwrite check on the host, history_gather_kernel (join_kernels.hip) and
// the envelope, quantile, extremes and events kernels (envelope_kernels.hip, quantile_kernels.hip, extremes_kernels.hip, events_kernels.hip) on the device, the fake runtime's
// launchers (hip_fake.cpp).
// history_plan_test.cpp checks it on the host.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define SIXDOF_HOST_DEVICE __host__ __device__
#else
#define SIXDOF_HOST_DEVICE
#endif

namespace sixdof {

// Ring slot of tick `tick` (1-based count of completed ticks): what the step kernel (step_kernel.hpp, hist_slot0 + tick) and
// snapshot_tick_to_ring write, and sixdof_history_read reads.
SIXDOF_HOST_DEVICE inline uint64_t history_slot(uint64_t tick, uint64_t ring) { return (tick - 1) % ring; }

// Slot of sample j of a range that starts at first_tick and takes every `every`-th tick.  The caller has validated the range
// (sampled_range_ok), so first_tick + j * every is at most the handle's tick and cannot wrap 64 bits.
SIXDOF_HOST_DEVICE inline uint64_t sample_slot(uint64_t first_tick, uint64_t j, uint64_t every, uint64_t ring) {
    return history_slot(first_tick + j * every, ring);
}

// The slot of the sample after the one in `slot`, without a division: step = every % ring.  What a thread that walks a whole
// range calls per sample (extremes_kernels.hip, events_kernels.hip); equal to sample_slot of the next index.
SIXDOF_HOST_DEVICE inline uint64_t next_sample_slot(uint64_t slot, uint64_t step, uint64_t ring) {
    slot += step;     // both below ring <= 2^32
    return slot >= ring ? slot - ring : slot;
}

// Whether the n_samples >= 1 ticks first_tick, first_tick + every, ... are all in a ring of `ring` slots that has recorded
// since `hist_first_tick` on a handle that has completed `tick` ticks: every >= 1, every sampled tick in
// [hist_first_tick, tick], and the oldest of them not yet overwritten (first_tick + ring > tick).  No step of it overflows.
inline bool sampled_range_ok(uint64_t first_tick, uint64_t n_samples, uint64_t every, uint64_t hist_first_tick, uint64_t tick,
                             uint64_t ring) {
    if (ring == 0 || every == 0 || n_samples == 0) return false;
    if (first_tick == 0 || first_tick < hist_first_tick || first_tick > tick) return false;
    if (tick - first_tick >= ring) return false;                      // first_tick + ring <= tick: overwritten
    return n_samples - 1 <= (tick - first_tick) / every;              // the last sample is at most `tick`
}

}  // namespace sixdof
