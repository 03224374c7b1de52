// extremes_kernels.hip — ring extremes: per row and component element, over the sampled ticks of a range, count / min / tick of
// min / max / tick of max / first non-finite tick, reduced on the device so that six numbers per element cross the link once,
// not every row of every tick.
//
// Ring of component k: [ring][n, w_k] blocks in the reference row layout.  One tick of one component is n * w contiguous
// elements; record, rule and segment cut are extremes_plan.hpp's, shared with the host twin.
//
// Stage 1, extremes_walk_kernel: grid (ceil(n * w / 256), segments, components).  One thread owns element i of the flat tick
// block and walks the samples of its segment in time order; consecutive lanes read consecutive elements, so a wave load is 512
// contiguous bytes of f64 (256 of f32), as in the envelope.  The loop is time_scan.hpp's scan_walk, which loads ahead of its use.
// The record lives in registers on integer keys; the finite test looks at the exponent bits.  With one segment the thread
// merges the accumulator of a continuing call in front of its record and writes the six planes itself; with more, its record
// goes to scratch, field-major so that the stores stay coalesced.
// Stage 2, extremes_merge_kernel (only with more than one segment): one thread per element folds the accumulator (continuing
// call) and the records of segments 0, 1, 2, ... in that order and writes the six planes.
// No floating-point arithmetic, no atomics.  All index arithmetic is 64-bit: slot * n * w passes 2^32 at 65,536 rows and a few
// thousand slots.
#include "extremes_plan.hpp"
#include "kernels.hpp"

namespace sixdof {

template <class E>
__global__ __launch_bounds__(kExtremesThreads) void extremes_walk_kernel(RingBinArgs a, double* __restrict__ out, uint64_t* __restrict__ scratch,
                                                                         uint64_t stride, uint32_t segments, uint32_t merge_into, uint64_t n,
                                                                         uint64_t first_tick, uint64_t n_samples, uint64_t every, uint64_t ring) {
    const RingBinDesc d = a.c[blockIdx.z];
    const uint64_t total = n * d.w;
    const uint64_t i = (uint64_t)blockIdx.x * kExtremesThreads + threadIdx.x;
    if (i >= total) return;      // a narrower component than the one that sized the grid, or the ragged last block
    const uint32_t seg = blockIdx.y;
    const uint64_t lo = scan_segment_start(n_samples, segments, seg), hi = scan_segment_start(n_samples, segments, seg + 1);
    ExtremesRecord r = scan_walk(extremes_empty(), ExtremesRule{}, static_cast<const E*>(d.ring) + i, total, lo, hi, first_tick, every, ring);
    if (segments == 1) {
        double* __restrict__ o = out + d.out_offset + i;
        if (merge_into) r = extremes_merge(extremes_absorb<E>(o, total), r);
        extremes_emit<E>(r, o, total);
    } else {
        extremes_store(r, scratch + (uint64_t)seg * kExtremesFields * stride + d.scratch_offset + i, stride);
    }
}

template <class E>
__global__ __launch_bounds__(kExtremesThreads) void extremes_merge_kernel(RingBinArgs a, double* __restrict__ out, const uint64_t* __restrict__ scratch,
                                                                          uint64_t stride, uint32_t segments, uint32_t merge_into, uint64_t n) {
    const RingBinDesc d = a.c[blockIdx.z];
    const uint64_t total = n * d.w;
    const uint64_t i = (uint64_t)blockIdx.x * kExtremesThreads + threadIdx.x;
    if (i >= total) return;
    double* __restrict__ o = out + d.out_offset + i;
    ExtremesRecord r = merge_into ? extremes_absorb<E>(o, total) : extremes_empty();
    const uint64_t* __restrict__ p = scratch + d.scratch_offset + i;
    for (uint32_t s = 0; s < segments; s++) r = extremes_merge(r, extremes_load(p + (uint64_t)s * kExtremesFields * stride, stride));
    extremes_emit<E>(r, o, total);
}

template <class E>
static hipError_t launch_extremes_as(const RingBinArgs& a, dim3 grid, double* out, uint64_t* scratch, uint64_t stride, uint32_t segments,
                                     uint32_t merge_into, uint64_t n, uint64_t first_tick, uint64_t n_samples, uint64_t every, uint64_t ring,
                                     hipStream_t s) {
    hipLaunchKernelGGL(extremes_walk_kernel<E>, grid, dim3(kExtremesThreads), 0, s, a, out, scratch, stride, segments, merge_into, n, first_tick, n_samples,
                       every, ring);
    if (hipError_t e = hipGetLastError(); e != hipSuccess || segments == 1) return e;
    hipLaunchKernelGGL(extremes_merge_kernel<E>, dim3(grid.x, 1, grid.z), dim3(kExtremesThreads), 0, s, a, out, scratch, stride, segments, merge_into, n);
    return hipGetLastError();
}

hipError_t launch_history_extremes(const RingBinArgs& a, uint32_t n_components, double* out, void* scratch, uint64_t scratch_stride,
                                   uint32_t segments, bool merge_into, uint64_t n, uint64_t first_tick, uint64_t n_samples, uint64_t every,
                                   uint64_t ring, size_t elem, hipStream_t s) {
    uint32_t widths[kRingBinMaxComponents] = {};
    for (uint32_t k = 0; k < n_components && k < kRingBinMaxComponents; k++) widths[k] = a.c[k].w;
    if (!extremes_launch_ok(n_components, kRingBinMaxComponents, widths, n, first_tick, n_samples, every, segments) || ring == 0)
        return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    uint64_t widest = 0;
    for (uint32_t k = 0; k < n_components; k++) widest = n * widths[k] > widest ? n * widths[k] : widest;
    const dim3 grid(static_cast<unsigned>((widest + kExtremesThreads - 1) / kExtremesThreads), segments, n_components);
    uint64_t* rec = static_cast<uint64_t*>(scratch);
    return elem == 8 ? launch_extremes_as<double>(a, grid, out, rec, scratch_stride, segments, merge_into, n, first_tick, n_samples, every, ring, s)
                     : launch_extremes_as<float>(a, grid, out, rec, scratch_stride, segments, merge_into, n, first_tick, n_samples, every, ring, s);
}

}  // namespace sixdof
