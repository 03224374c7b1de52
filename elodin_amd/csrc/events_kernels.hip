// events_kernels.hip — ring events: per trigger and run, the first sampled tick at which one element of one recorded component
// meets a threshold (x op level, as a level or as a crossing), the element's value there and at the finite sample before, and
// the rows of other components at that tick — found and captured on the device, in the call that sees the event, so that a
// handful of numbers per run cross the link once.
//
// Ring of a component: [ring][n, w] blocks in the reference row layout.  A run is `period` consecutive rows; a trigger reads
// element `element` of row run * period + group.  Record, rule and segment cut are events_plan.hpp's, shared with the host twin.
//
// Stage 1, events_walk_kernel: grid (ceil(runs / 256), segments, triggers).  One thread owns one run and walks the samples of its
// segment in time order.  Consecutive lanes are period * w elements apart: at period 1 a wave's load touches a contiguous span of
// 64 * w elements and uses 1 / w of it (one f64 in seven of world_pos: 512 of 3,584 bytes), at a larger period 1 / (period * w)
// — the price of reading one element of a row-major block; the cache lines are the ones a reader of whole rows would fetch
// once.  The loop is time_scan.hpp's scan_walk written out (see below): kScanLoads samples are loaded before the first is used, the
// slot advances by an add and a compare.  A thread whose record is settled (events_settled) stops loading;
// a wave goes on while any of its lanes does.  With one segment the thread starts from the accumulator's record of a continuing
// call — by the rule's associativity the same as merging it in front of its own, and a run that has had its event loads nothing
// — stores the record and writes the four planes; with more, its record goes to scratch, field-major so that the stores stay
// coalesced.
// Stage 2, events_merge_kernel (only with more than one segment): one thread per (run, trigger) folds the accumulator's record
// (continuing call) and the records of segments 0, 1, 2, ... in that order, stores the record and writes the four planes.
// Stage 3, events_capture_kernel: grid (ceil(n * w / 256), triggers, captured components).  Element i of the flat [n * w] block
// belongs to run (i / w) / period; where that run's event tick for the trigger is one of THIS call's samples, out[trigger][i] is
// the ring's element at that tick, widened to double.  The tick is checked against the call's range (events_tick_sampled) before
// a slot is formed of it.  Otherwise a fresh call writes NaN and a continuing call leaves the element alone.  Consecutive lanes
// read consecutive elements of a row.
// No atomics; no floating-point arithmetic beyond the compare and the widening.  All index arithmetic is 64-bit.
#include "events_plan.hpp"
#include "kernels.hpp"

namespace sixdof {

template <class E>
__global__ __launch_bounds__(kEventsThreads) void events_walk_kernel(EventsArgs a, uint64_t* __restrict__ rec, double* __restrict__ out,
                                                                     uint64_t* __restrict__ scratch, uint32_t segments, uint32_t merge_into,
                                                                     uint64_t n, uint32_t period, uint64_t first_tick, uint64_t n_samples,
                                                                     uint64_t every, uint64_t ring) {
    const EventsTrigger t = a.t[blockIdx.z];
    const uint64_t runs = n / period;
    const uint64_t run = (uint64_t)blockIdx.x * kEventsThreads + threadIdx.x;
    if (run >= runs) return;
    const uint32_t seg = blockIdx.y, trig = blockIdx.z, n_triggers = gridDim.z;
    const uint64_t lo = scan_segment_start(n_samples, segments, seg), hi = scan_segment_start(n_samples, segments, seg + 1);
    const uint64_t total = n * t.w;
    const E* __restrict__ src = static_cast<const E*>(t.ring) + (run * period + t.group) * t.w + t.element;
    const uint64_t step = every % ring;
    uint64_t slot = sample_slot(first_tick, lo, every, ring), tick = first_tick + lo * every;
    uint64_t* __restrict__ mine = rec + (uint64_t)trig * kEventsFields * runs + run;
    EventsRecord r = segments == 1 && merge_into ? events_load(mine, runs) : events_empty();
    // scan_walk's loop, written out: through scan_walk this kernel measured about 1 % slower where a thread's chain is long
    // (profiles/time_scan_refactor.md).  The host twin runs scan_walk with EventsRule; events_host_test holds the two together.
    uint64_t j = lo;
    for (; j + kScanLoads <= hi && !events_settled(r, t.mode); j += kScanLoads) {
        E x[kScanLoads];
#pragma unroll
        for (uint32_t q = 0; q < kScanLoads; q++) {
            x[q] = src[slot * total];
            slot = next_sample_slot(slot, step, ring);
        }
#pragma unroll
        for (uint32_t q = 0; q < kScanLoads; q++) {
            events_sample<E>(r, x[q], tick, t.op, t.level);
            tick += every;
        }
    }
    for (; j < hi && !events_settled(r, t.mode); j++) {
        events_sample<E>(r, src[slot * total], tick, t.op, t.level);
        slot = next_sample_slot(slot, step, ring);
        tick += every;
    }
    if (segments == 1) {
        events_store(r, mine, runs);
        events_emit<E>(r, t.mode, out + (uint64_t)trig * kEventsPlanes * runs + run, runs);
    } else {
        events_store(r, scratch + ((uint64_t)seg * n_triggers + trig) * kEventsFields * runs + run, runs);
    }
}

template <class E>
__global__ __launch_bounds__(kEventsThreads) void events_merge_kernel(EventsArgs a, uint64_t* __restrict__ rec, double* __restrict__ out,
                                                                      const uint64_t* __restrict__ scratch, uint32_t segments, uint32_t merge_into,
                                                                      uint64_t runs) {
    const uint64_t run = (uint64_t)blockIdx.x * kEventsThreads + threadIdx.x;
    if (run >= runs) return;
    const uint32_t trig = blockIdx.z, n_triggers = gridDim.z;
    uint64_t* __restrict__ mine = rec + (uint64_t)trig * kEventsFields * runs + run;
    EventsRecord r = merge_into ? events_load(mine, runs) : events_empty();
    for (uint32_t s = 0; s < segments; s++) r = events_merge(r, events_load(scratch + ((uint64_t)s * n_triggers + trig) * kEventsFields * runs + run, runs));
    events_store(r, mine, runs);
    events_emit<E>(r, a.t[trig].mode, out + (uint64_t)trig * kEventsPlanes * runs + run, runs);
}

template <class E>
__global__ __launch_bounds__(kEventsThreads) void events_capture_kernel(EventsArgs a, RingBinArgs c, const uint64_t* __restrict__ rec, double* __restrict__ out,
                                                                        uint32_t merge_into, uint64_t n, uint32_t period, uint64_t first_tick,
                                                                        uint64_t last, uint64_t every, uint64_t ring) {
    const RingBinDesc d = c.c[blockIdx.z];
    const uint64_t total = n * d.w;
    const uint64_t i = (uint64_t)blockIdx.x * kEventsThreads + threadIdx.x;
    if (i >= total) return;      // a narrower component than the one that sized the grid, or the ragged last block
    const uint32_t trig = blockIdx.y;
    const uint64_t runs = n / period, run = i / d.w / period;
    const uint64_t tick = events_stored_tick(rec + (uint64_t)trig * kEventsFields * runs + run, runs, a.t[trig].mode);
    double* __restrict__ o = out + d.out_offset + (uint64_t)trig * total + i;
    if (events_tick_sampled(tick, first_tick, last, every)) {
        *o = static_cast<double>(static_cast<const E*>(d.ring)[history_slot(tick, ring) * total + i]);
    } else if (!merge_into) {
        *o = __builtin_nan("");
    }
}

template <class E>
static hipError_t launch_events_as(const EventsArgs& a, dim3 grid, uint64_t* rec, double* out, uint64_t* scratch, uint32_t segments, uint32_t merge_into,
                                   uint64_t n, uint32_t period, uint64_t first_tick, uint64_t n_samples, uint64_t every, uint64_t ring, hipStream_t s) {
    hipLaunchKernelGGL(events_walk_kernel<E>, grid, dim3(kEventsThreads), 0, s, a, rec, out, scratch, segments, merge_into, n, period, first_tick, n_samples,
                       every, ring);
    if (hipError_t e = hipGetLastError(); e != hipSuccess || segments == 1) return e;
    hipLaunchKernelGGL(events_merge_kernel<E>, dim3(grid.x, 1, grid.z), dim3(kEventsThreads), 0, s, a, rec, out, scratch, segments, merge_into, n / period);
    return hipGetLastError();
}

hipError_t launch_history_events(const EventsArgs& a, uint32_t n_triggers, void* rec, double* out, void* scratch, uint32_t segments, bool merge_into,
                                 uint64_t n, uint32_t period, uint64_t first_tick, uint64_t n_samples, uint64_t every, uint64_t ring, size_t elem,
                                 hipStream_t s) {
    if (!events_launch_ok(a, n_triggers, n, period, first_tick, n_samples, every, segments) || ring == 0) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    const dim3 grid(static_cast<unsigned>((n / period + kEventsThreads - 1) / kEventsThreads), segments, n_triggers);
    uint64_t *r = static_cast<uint64_t*>(rec), *sc = static_cast<uint64_t*>(scratch);
    return elem == 8 ? launch_events_as<double>(a, grid, r, out, sc, segments, merge_into, n, period, first_tick, n_samples, every, ring, s)
                     : launch_events_as<float>(a, grid, r, out, sc, segments, merge_into, n, period, first_tick, n_samples, every, ring, s);
}

hipError_t launch_events_capture(const EventsArgs& a, uint32_t n_triggers, const RingBinArgs& c, uint32_t n_captures, const void* rec, double* out,
                                 bool merge_into, uint64_t n, uint32_t period, uint64_t first_tick, uint64_t n_samples, uint64_t every, uint64_t ring,
                                 size_t elem, hipStream_t s) {
    uint32_t widths[kRingBinMaxComponents] = {};
    for (uint32_t k = 0; k < n_captures && k < kRingBinMaxComponents; k++) widths[k] = c.c[k].w;
    if (!events_capture_ok(a, n_triggers, n_captures, kRingBinMaxComponents, widths, n, period, first_tick, n_samples, every) || ring == 0)
        return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    uint64_t widest = 0;
    for (uint32_t k = 0; k < n_captures; k++) widest = n * widths[k] > widest ? n * widths[k] : widest;
    const dim3 grid(static_cast<unsigned>((widest + kEventsThreads - 1) / kEventsThreads), n_triggers, n_captures);
    const uint64_t last = first_tick + (n_samples - 1) * every;
    const uint64_t* r = static_cast<const uint64_t*>(rec);
    if (elem == 8)
        hipLaunchKernelGGL(events_capture_kernel<double>, grid, dim3(kEventsThreads), 0, s, a, c, r, out, uint32_t(merge_into), n, period, first_tick, last, every, ring);
    else
        hipLaunchKernelGGL(events_capture_kernel<float>, grid, dim3(kEventsThreads), 0, s, a, c, r, out, uint32_t(merge_into), n, period, first_tick, last, every, ring);
    return hipGetLastError();
}

}  // namespace sixdof
