// envelope_kernels.hip — ring envelopes: per sampled tick and component element, count / min / max / mean / m2 over the rows
// of one group (row % period), reduced on the device so that five numbers per element and tick cross the link, not n rows.
//
// Ring of component k: [ring][n, w_k] blocks in the reference row layout (join_kernels.hip, history_gather_kernel).  One tick of
// one component is n * w contiguous elements, element i in bin i % (period * w) — geometry, accumulation and merge order are
// envelope_plan.hpp's, shared with the host twin.
//
// Stage 1, envelope_partial_kernel: grid (blocks, samples, components).  Thread t of a block reads element tile * g.tile + t of
// the tiles dealt to its block: consecutive lanes read consecutive elements (a wave reads 512 contiguous bytes of f64, 256 of
// f32), and because g.tile is a multiple of the bin count the thread stays on bin t % bins and keeps one accumulator in
// registers.  A wider load per lane would put a lane on several bins (the bin pattern has period 7 for world_pos) and needs the
// tick block 16-byte aligned, which n * 7 * 8 bytes is for even n only; instead four tiles are loaded before the first is
// used, so four loads per lane are in flight.  Nothing is read twice: LDS only combines the per_bin threads that share a bin,
// as a binary tree in a fixed order.  Each block writes `bins` records; no atomics.
// Stage 2, envelope_merge_kernel: one thread per (sample, component, bin) merges the records of blocks 0, 1, 2, ... in that
// order and writes the five output values.
// All index arithmetic is 64-bit: slot * n * w passes 2^32 at 65,536 rows and a few thousand slots.
#include "envelope_plan.hpp"
#include "kernels.hpp"

namespace sixdof {

template <class E>
__global__ __launch_bounds__(kEnvelopeThreads) void envelope_partial_kernel(RingBinArgs a, EnvelopePartial* __restrict__ partial,
                                                                            uint64_t partial_stride, uint64_t n, uint32_t period,
                                                                            uint64_t first_tick, uint64_t sample0, uint64_t every,
                                                                            uint64_t ring) {
    __shared__ EnvelopePartial rec[kEnvelopeThreads];
    const RingBinDesc d = a.c[blockIdx.z];
    const EnvelopeGeom g = envelope_geom(n, d.w, period);
    const uint32_t b = blockIdx.x, t = threadIdx.x;
    if (b >= g.blocks) return;   // a narrower component than the one that sized the grid: the whole block leaves
    const uint64_t total = n * d.w;
    const uint64_t slot = sample_slot(first_tick, sample0 + blockIdx.y, every, ring);
    const E* __restrict__ src = static_cast<const E*>(d.ring) + slot * total;
    EnvelopePartial acc = envelope_empty();
    if (t < g.tile) {
        const uint64_t step = (uint64_t)g.blocks * g.tile;
        uint64_t i = (uint64_t)b * g.tile + t;
        for (; i + 3 * step < total; i += 4 * step) {
            const E x0 = src[i], x1 = src[i + step], x2 = src[i + 2 * step], x3 = src[i + 3 * step];
            envelope_accumulate(acc, (double)x0);
            envelope_accumulate(acc, (double)x1);
            envelope_accumulate(acc, (double)x2);
            envelope_accumulate(acc, (double)x3);
        }
        for (; i < total; i += step) envelope_accumulate(acc, (double)src[i]);
    }
    rec[t] = acc;
    __syncthreads();
    const uint32_t j = t / g.bins;   // the t >= g.tile threads hold empty records and j >= per_bin: they only meet the barriers
    for (uint32_t s = envelope_tree_start(g.per_bin); s >= 1; s /= 2) {
        if (j < s && j + s < g.per_bin) rec[t] = envelope_merge(rec[t], rec[t + s * g.bins]);
        __syncthreads();
    }
    if (t < g.bins) partial[(uint64_t)blockIdx.y * partial_stride + d.scratch_offset + (uint64_t)b * g.bins + t] = rec[t];
}

__global__ __launch_bounds__(128) void envelope_merge_kernel(RingBinArgs a, const EnvelopePartial* __restrict__ partial,
                                                             uint64_t partial_stride, double* __restrict__ out, uint64_t n,
                                                             uint32_t period, uint64_t sample0) {
    const RingBinDesc d = a.c[blockIdx.z];
    const EnvelopeGeom g = envelope_geom(n, d.w, period);
    const uint32_t bin = blockIdx.x * blockDim.x + threadIdx.x;
    if (bin >= g.bins) return;
    const EnvelopePartial* __restrict__ p = partial + (uint64_t)blockIdx.y * partial_stride + d.scratch_offset + bin;
    EnvelopePartial r = p[0];
    for (uint32_t b = 1; b < g.blocks; b++) r = envelope_merge(r, p[(uint64_t)b * g.bins]);
    const uint64_t group = bin / d.w, c = bin % d.w, sample = sample0 + blockIdx.y;
    envelope_emit(r, out + d.out_offset + ((sample * period + group) * kEnvelopeStats) * d.w + c, d.w);
}

hipError_t launch_history_envelope(const RingBinArgs& a, uint32_t n_components, double* out, void* partial, uint64_t partial_stride,
                                   uint64_t n, uint32_t period, uint64_t first_tick, uint64_t sample0, uint64_t n_samples,
                                   uint64_t every, uint64_t ring, size_t elem, hipStream_t s) {
    if (!envelope_launch_ok(n_components, kRingBinMaxComponents, n_samples, period)) return hipErrorInvalidValue;
    if (n_samples == 0 || n == 0) return hipSuccess;
    uint32_t blocks = 0, bins = 0;
    for (uint32_t k = 0; k < n_components; k++) {
        if (!envelope_supported(a.c[k].w, period)) return hipErrorInvalidValue;
        const EnvelopeGeom g = envelope_geom(n, a.c[k].w, period);
        blocks = g.blocks > blocks ? g.blocks : blocks;
        bins = g.bins > bins ? g.bins : bins;
    }
    EnvelopePartial* rec = static_cast<EnvelopePartial*>(partial);
    const dim3 grid1(blocks, (unsigned)n_samples, n_components), grid2((bins + 127) / 128, (unsigned)n_samples, n_components);
    if (elem == 8) hipLaunchKernelGGL(envelope_partial_kernel<double>, grid1, dim3(kEnvelopeThreads), 0, s, a, rec, partial_stride, n, period, first_tick, sample0, every, ring);
    else hipLaunchKernelGGL(envelope_partial_kernel<float>, grid1, dim3(kEnvelopeThreads), 0, s, a, rec, partial_stride, n, period, first_tick, sample0, every, ring);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(envelope_merge_kernel, grid2, dim3(128), 0, s, a, rec, partial_stride, out, n, period, sample0);
    return hipGetLastError();
}

}  // namespace sixdof
