// dwell_kernels.hip — ring dwell: per condition and run, over the sampled ticks of a range, how long and how often a predicate on
// one element, on a difference of two elements or on the squared length of a small vector of the ring held — time above a load
// limit, excursions out of a corridor, time inside a keep-out sphere, the longest unbroken stretch above a tumble limit — reduced
// on the device so that twelve numbers per condition and run cross the link once.
//
// Ring of a component: [ring][n, w] blocks in the reference row layout.  A run is `period` consecutive rows; record, rule, value,
// walk and segment cut are dwell_plan.hpp's (the walk and the squared norm norms_plan.hpp's), all shared with the host twin.
//
// Stage 1, dwell_walk_kernel: grid (ceil(runs / 256), segments, conditions).  One thread owns one (condition, run) and walks the
// samples of its segment in time order (dwell_walk): the loads of norms_depth samples are issued before the first value is
// formed.  Consecutive lanes are period * w elements apart, as in the norms' walk.  The value is formed in f64 without FMA
// contraction, compared against the levels, and the record — twelve integers, updated by selects — stays in registers.  With one
// segment the thread merges the accumulator of a continuing call in front of its record and writes the twelve planes itself;
// with more, its record goes to scratch, field-major so that the stores stay coalesced.
// Stage 2, dwell_merge_kernel (only with more than one segment): one thread per (condition, run) folds the accumulator
// (continuing call) and the records of segments 0, 1, 2, ... in that order and writes the twelve planes.
// No atomics, no LDS.  All index arithmetic is 64-bit.
#include "dwell_plan.hpp"
#include "kernels.hpp"

namespace sixdof {

template <class E>
__global__ __launch_bounds__(kDwellThreads) void dwell_walk_kernel(DwellArgs a, double* __restrict__ out, uint64_t* __restrict__ scratch, uint32_t segments,
                                                                   uint32_t merge_into, uint64_t n, uint32_t period, uint64_t first_tick,
                                                                   uint64_t n_samples, uint64_t every, uint64_t ring) {
    const DwellCondition c = a.c[blockIdx.z];
    const uint64_t runs = n / period;
    const uint64_t run = (uint64_t)blockIdx.x * kDwellThreads + threadIdx.x;
    if (run >= runs) return;
    const uint32_t seg = blockIdx.y, cond = blockIdx.z, n_conditions = gridDim.z;
    const uint64_t lo = scan_segment_start(n_samples, segments, seg), hi = scan_segment_start(n_samples, segments, seg + 1);
    DwellRecord r = dwell_walk<E>(dwell_empty(), c, run, n, period, lo, hi, first_tick, every, ring);
    if (segments == 1) {
        double* __restrict__ o = out + dwell_out_index(cond, runs, run);
        if (merge_into) r = dwell_merge(dwell_absorb(o, runs), r);
        dwell_emit(r, o, runs);
    } else {
        dwell_store(r, scratch + dwell_scratch_index(seg, n_conditions, cond, runs, run), runs);
    }
}

__global__ __launch_bounds__(kDwellThreads) void dwell_merge_kernel(double* __restrict__ out, const uint64_t* __restrict__ scratch, uint32_t segments,
                                                                    uint32_t merge_into, uint64_t runs) {
    const uint64_t run = (uint64_t)blockIdx.x * kDwellThreads + threadIdx.x;
    if (run >= runs) return;
    const uint32_t cond = blockIdx.z, n_conditions = gridDim.z;
    double* __restrict__ o = out + dwell_out_index(cond, runs, run);
    DwellRecord r = merge_into ? dwell_absorb(o, runs) : dwell_empty();
    for (uint32_t s = 0; s < segments; s++) r = dwell_merge(r, dwell_load(scratch + dwell_scratch_index(s, n_conditions, cond, runs, run), runs));
    dwell_emit(r, o, runs);
}

template <class E>
static hipError_t launch_dwell_as(const DwellArgs& a, dim3 grid, double* out, uint64_t* scratch, uint32_t segments, uint32_t merge_into, uint64_t n,
                                  uint32_t period, uint64_t first_tick, uint64_t n_samples, uint64_t every, uint64_t ring, hipStream_t s) {
    hipLaunchKernelGGL(dwell_walk_kernel<E>, grid, dim3(kDwellThreads), 0, s, a, out, scratch, segments, merge_into, n, period, first_tick, n_samples, every, ring);
    if (hipError_t e = hipGetLastError(); e != hipSuccess || segments == 1) return e;
    hipLaunchKernelGGL(dwell_merge_kernel, dim3(grid.x, 1, grid.z), dim3(kDwellThreads), 0, s, out, scratch, segments, merge_into, n / period);
    return hipGetLastError();
}

hipError_t launch_history_dwell(const DwellArgs& a, uint32_t n_conditions, double* out, void* scratch, uint32_t segments, bool merge_into, uint64_t n,
                                uint32_t period, uint64_t first_tick, uint64_t n_samples, uint64_t every, uint64_t ring, size_t elem, hipStream_t s) {
    if (!dwell_launch_ok(a, n_conditions, n, period, first_tick, n_samples, every, segments) || ring == 0) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    const dim3 grid(static_cast<unsigned>((n / period + kDwellThreads - 1) / kDwellThreads), segments, n_conditions);
    uint64_t* sc = static_cast<uint64_t*>(scratch);
    return elem == 8 ? launch_dwell_as<double>(a, grid, out, sc, segments, merge_into, n, period, first_tick, n_samples, every, ring, s)
                     : launch_dwell_as<float>(a, grid, out, sc, segments, merge_into, n, period, first_tick, n_samples, every, ring, s);
}

}  // namespace sixdof
