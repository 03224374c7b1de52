// norms_kernels.hip — ring norms: per probe and run, over the sampled ticks of a range, the extremes of the squared length of a
// small vector of the ring — |r|, |v|, |omega|, |q| — or of the separation of two rows of a run, with the ticks they fall on,
// reduced on the device so that six numbers per probe and run cross the link once.
//
// Ring of a component: [ring][n, w] blocks in the reference row layout.  A run is `period` consecutive rows; probe, value, walk
// and segment cut are norms_plan.hpp's, the record and the rule extremes_plan.hpp's, all shared with the host twin.
//
// Stage 1, norms_walk_kernel: grid (ceil(runs / 256), segments, probes).  One thread owns one (probe, run) and walks the samples
// of its segment in time order (norms_walk): per sample count loads from row A and, with MINUS, count from row B, all of
// norms_depth samples issued before the first square is formed.  Consecutive lanes are period * w elements apart, as in the
// events' walk; a probe uses count of the w elements a lane's cache line holds.  The squared norm is formed in f64 without FMA
// contraction and goes to the rule as an integer key.  With one segment the thread merges the accumulator of a continuing
// call in front of its record and writes the six planes itself; with more, its record goes to scratch, field-major so that the
// stores stay coalesced.
// Stage 2, norms_merge_kernel (only with more than one segment): one thread per (probe, run) folds the accumulator (continuing
// call) and the records of segments 0, 1, 2, ... in that order and writes the six planes.
// No atomics, no LDS.  All index arithmetic is 64-bit.
#include "norms_plan.hpp"
#include "kernels.hpp"

namespace sixdof {

template <class E>
__global__ __launch_bounds__(kNormsThreads) void norms_walk_kernel(NormsArgs a, double* __restrict__ out, uint64_t* __restrict__ scratch, uint32_t segments,
                                                                   uint32_t merge_into, uint64_t n, uint32_t period, uint64_t first_tick,
                                                                   uint64_t n_samples, uint64_t every, uint64_t ring) {
    const NormsProbe p = a.p[blockIdx.z];
    const uint64_t runs = n / period;
    const uint64_t run = (uint64_t)blockIdx.x * kNormsThreads + threadIdx.x;
    if (run >= runs) return;
    const uint32_t seg = blockIdx.y, probe = blockIdx.z, n_probes = gridDim.z;
    const uint64_t lo = scan_segment_start(n_samples, segments, seg), hi = scan_segment_start(n_samples, segments, seg + 1);
    ExtremesRecord r = norms_walk<E>(extremes_empty(), p, run, n, period, lo, hi, first_tick, every, ring);
    if (segments == 1) {
        double* __restrict__ o = out + norms_out_index(probe, runs, run);
        if (merge_into) r = extremes_merge(extremes_absorb<double>(o, runs), r);
        extremes_emit<double>(r, o, runs);
    } else {
        extremes_store(r, scratch + norms_scratch_index(seg, n_probes, probe, runs, run), runs);
    }
}

__global__ __launch_bounds__(kNormsThreads) void norms_merge_kernel(double* __restrict__ out, const uint64_t* __restrict__ scratch, uint32_t segments,
                                                                    uint32_t merge_into, uint64_t runs) {
    const uint64_t run = (uint64_t)blockIdx.x * kNormsThreads + threadIdx.x;
    if (run >= runs) return;
    const uint32_t probe = blockIdx.z, n_probes = gridDim.z;
    double* __restrict__ o = out + norms_out_index(probe, runs, run);
    ExtremesRecord r = merge_into ? extremes_absorb<double>(o, runs) : extremes_empty();
    for (uint32_t s = 0; s < segments; s++) r = extremes_merge(r, extremes_load(scratch + norms_scratch_index(s, n_probes, probe, runs, run), runs));
    extremes_emit<double>(r, o, runs);
}

template <class E>
static hipError_t launch_norms_as(const NormsArgs& a, dim3 grid, double* out, uint64_t* scratch, uint32_t segments, uint32_t merge_into, uint64_t n,
                                  uint32_t period, uint64_t first_tick, uint64_t n_samples, uint64_t every, uint64_t ring, hipStream_t s) {
    hipLaunchKernelGGL(norms_walk_kernel<E>, grid, dim3(kNormsThreads), 0, s, a, out, scratch, segments, merge_into, n, period, first_tick, n_samples, every, ring);
    if (hipError_t e = hipGetLastError(); e != hipSuccess || segments == 1) return e;
    hipLaunchKernelGGL(norms_merge_kernel, dim3(grid.x, 1, grid.z), dim3(kNormsThreads), 0, s, out, scratch, segments, merge_into, n / period);
    return hipGetLastError();
}

hipError_t launch_history_norms(const NormsArgs& a, uint32_t n_probes, double* out, void* scratch, uint32_t segments, bool merge_into, uint64_t n,
                                uint32_t period, uint64_t first_tick, uint64_t n_samples, uint64_t every, uint64_t ring, size_t elem, hipStream_t s) {
    if (!norms_launch_ok(a, n_probes, n, period, first_tick, n_samples, every, segments) || ring == 0) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    const dim3 grid(static_cast<unsigned>((n / period + kNormsThreads - 1) / kNormsThreads), segments, n_probes);
    uint64_t* sc = static_cast<uint64_t*>(scratch);
    return elem == 8 ? launch_norms_as<double>(a, grid, out, sc, segments, merge_into, n, period, first_tick, n_samples, every, ring, s)
                     : launch_norms_as<float>(a, grid, out, sc, segments, merge_into, n, period, first_tick, n_samples, every, ring, s);
}

}  // namespace sixdof
