// norm_events_kernels.hip — ring norm events: per trigger and run, the first sampled tick at which the squared length of a small
// vector of the ring — |r|, |v|, |omega|, |q| — or of the separation of two rows of a run meets a squared level (s op level_sq, as a
// level or as a crossing), with s there and at the finite sample before — found on the device, in the call that sees the event, so
// that a handful of numbers per run cross the link once.  The rows of other components at that tick are captured behind it by
// events_kernels.hip's capture stage, unchanged: the record buffer has the events' layout.
//
// Ring of a component: [ring][n, w] blocks in the reference row layout.  A run is `period` consecutive rows; trigger, rule and
// geometry are norm_events_plan.hpp's, the value and the walk norms_plan.hpp's, the record events_plan.hpp's, all shared with the
// host twin.
//
// Stage 1, norm_events_walk_kernel: grid (ceil(runs / 256), segments, triggers).  One thread owns one (trigger, run) and walks the
// samples of its segment in time order (norm_events_walk, the norms' walk under the events' rule): per sample count loads from
// row A and, with MINUS, count from row B, all of norms_depth samples — at most 16 elements — issued before the first square is
// formed; the switch on (count, MINUS) is uniform per block.  A thread whose record is settled (events_settled) stops loading; a
// wave goes on while any of its lanes does.  With one segment the thread starts from the accumulator's record of a continuing
// call — by the rule's associativity the same as merging it in front of its own, and a run that has had its event loads nothing
// — stores the record and writes the four planes; with more, its record goes to scratch, field-major so that the stores stay
// coalesced.
// Stage 2, norm_events_merge_kernel (only with more than one segment): one thread per (run, trigger) folds the accumulator's
// record (continuing call) and the records of segments 0, 1, 2, ... in that order, stores the record and writes the four planes.
// No atomics, no LDS; no floating-point beyond norms_value, the compare and the widening.  All index arithmetic is 64-bit.
#include "norm_events_plan.hpp"
#include "kernels.hpp"

namespace sixdof {

template <class E>
__global__ __launch_bounds__(kNormEventsThreads) void norm_events_walk_kernel(NormEventsArgs a, uint64_t* __restrict__ rec, double* __restrict__ out,
                                                                              uint64_t* __restrict__ scratch, uint32_t segments, uint32_t merge_into,
                                                                              uint64_t n, uint32_t period, uint64_t first_tick, uint64_t n_samples,
                                                                              uint64_t every, uint64_t ring) {
    const NormEventsTrigger t = a.t[blockIdx.z];
    const uint64_t runs = n / period;
    const uint64_t run = (uint64_t)blockIdx.x * kNormEventsThreads + threadIdx.x;
    if (run >= runs) return;
    const uint32_t seg = blockIdx.y, trig = blockIdx.z, n_triggers = gridDim.z;
    const uint64_t lo = scan_segment_start(n_samples, segments, seg), hi = scan_segment_start(n_samples, segments, seg + 1);
    uint64_t* __restrict__ mine = rec + norm_events_record_index(trig, runs, run);
    EventsRecord r = segments == 1 && merge_into ? events_load(mine, runs) : events_empty();
    r = norm_events_walk<E>(r, t, run, n, period, lo, hi, first_tick, every, ring);
    if (segments == 1) {
        events_store(r, mine, runs);
        events_emit<double>(r, t.mode, out + norm_events_out_index(trig, runs, run), runs);
    } else {
        events_store(r, scratch + norm_events_scratch_index(seg, n_triggers, trig, runs, run), runs);
    }
}

__global__ __launch_bounds__(kNormEventsThreads) void norm_events_merge_kernel(NormEventsArgs a, uint64_t* __restrict__ rec, double* __restrict__ out,
                                                                               const uint64_t* __restrict__ scratch, uint32_t segments, uint32_t merge_into,
                                                                               uint64_t runs) {
    const uint64_t run = (uint64_t)blockIdx.x * kNormEventsThreads + threadIdx.x;
    if (run >= runs) return;
    const uint32_t trig = blockIdx.z, n_triggers = gridDim.z;
    uint64_t* __restrict__ mine = rec + norm_events_record_index(trig, runs, run);
    EventsRecord r = merge_into ? events_load(mine, runs) : events_empty();
    for (uint32_t s = 0; s < segments; s++) r = events_merge(r, events_load(scratch + norm_events_scratch_index(s, n_triggers, trig, runs, run), runs));
    events_store(r, mine, runs);
    events_emit<double>(r, a.t[trig].mode, out + norm_events_out_index(trig, runs, run), runs);
}

template <class E>
static hipError_t launch_norm_events_as(const NormEventsArgs& a, dim3 grid, uint64_t* rec, double* out, uint64_t* scratch, uint32_t segments, uint32_t merge_into,
                                        uint64_t n, uint32_t period, uint64_t first_tick, uint64_t n_samples, uint64_t every, uint64_t ring, hipStream_t s) {
    hipLaunchKernelGGL(norm_events_walk_kernel<E>, grid, dim3(kNormEventsThreads), 0, s, a, rec, out, scratch, segments, merge_into, n, period, first_tick,
                       n_samples, every, ring);
    if (hipError_t e = hipGetLastError(); e != hipSuccess || segments == 1) return e;
    hipLaunchKernelGGL(norm_events_merge_kernel, dim3(grid.x, 1, grid.z), dim3(kNormEventsThreads), 0, s, a, rec, out, scratch, segments, merge_into, n / period);
    return hipGetLastError();
}

hipError_t launch_history_norm_events(const NormEventsArgs& a, uint32_t n_triggers, void* rec, double* out, void* scratch, uint32_t segments, bool merge_into,
                                      uint64_t n, uint32_t period, uint64_t first_tick, uint64_t n_samples, uint64_t every, uint64_t ring, size_t elem,
                                      hipStream_t s) {
    if (!norm_events_launch_ok(a, n_triggers, n, period, first_tick, n_samples, every, segments) || ring == 0) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    const dim3 grid(static_cast<unsigned>((n / period + kNormEventsThreads - 1) / kNormEventsThreads), segments, n_triggers);
    uint64_t *r = static_cast<uint64_t*>(rec), *sc = static_cast<uint64_t*>(scratch);
    return elem == 8 ? launch_norm_events_as<double>(a, grid, r, out, sc, segments, merge_into, n, period, first_tick, n_samples, every, ring, s)
                     : launch_norm_events_as<float>(a, grid, r, out, sc, segments, merge_into, n, period, first_tick, n_samples, every, ring, s);
}

}  // namespace sixdof
