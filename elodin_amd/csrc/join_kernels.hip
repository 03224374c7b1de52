// join_kernels.hip — device gather / scatter by constant u32 row indices.
//
// Reference semantics (libs/nox-py/src/query.rs:136-208,599-725): a query over several components
// iterates the INTERSECTION of their entity-id sets in ascending id order; each component is gathered
// with a constant u32 index vector baked at compile time and results are scattered back by row
// (`dynamic_update_slice`).  Entities that carry only some of the components (static scene objects with a
// world_pos but no Body, examples/apollo-lander/sim.py:312-332) are never touched by six_dof.
// Here the joined rows live in compact [m,w] device columns that the step kernels update in place;
// gather runs after an upload, scatter before a download, so the per-tick path pays nothing.
#include "history_plan.hpp"
#include "kernels.hpp"

namespace sixdof {

template <class E>
__global__ __launch_bounds__(256) void gather_rows_kernel(E* __restrict__ dst, const E* __restrict__ src,
                                                          const uint32_t* __restrict__ rows, uint32_t m, uint32_t w) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)m * w) return;
    const uint32_t r = (uint32_t)(i / w), c = (uint32_t)(i % w);
    dst[i] = src[(uint64_t)rows[r] * w + c];
}

template <class E>
__global__ __launch_bounds__(256) void scatter_rows_kernel(E* __restrict__ dst, const E* __restrict__ src,
                                                           const uint32_t* __restrict__ rows, uint32_t m, uint32_t w) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)m * w) return;
    const uint32_t r = (uint32_t)(i / w), c = (uint32_t)(i % w);
    dst[(uint64_t)rows[r] * w + c] = src[i];
}

hipError_t launch_gather_rows(void* dst, const void* src, const uint32_t* rows, uint32_t m, uint32_t w, size_t elem,
                              hipStream_t s) {
    if (m == 0 || w == 0) return hipSuccess;
    const dim3 grid((unsigned)(((uint64_t)m * w + 255) / 256));
    if (elem == 8) hipLaunchKernelGGL(gather_rows_kernel<uint64_t>, grid, dim3(256), 0, s, (uint64_t*)dst, (const uint64_t*)src, rows, m, w);
    else hipLaunchKernelGGL(gather_rows_kernel<uint32_t>, grid, dim3(256), 0, s, (uint32_t*)dst, (const uint32_t*)src, rows, m, w);
    return hipGetLastError();
}

hipError_t launch_scatter_rows(void* dst, const void* src, const uint32_t* rows, uint32_t m, uint32_t w, size_t elem,
                               hipStream_t s) {
    if (m == 0 || w == 0) return hipSuccess;
    const dim3 grid((unsigned)(((uint64_t)m * w + 255) / 256));
    if (elem == 8) hipLaunchKernelGGL(scatter_rows_kernel<uint64_t>, grid, dim3(256), 0, s, (uint64_t*)dst, (const uint64_t*)src, rows, m, w);
    else hipLaunchKernelGGL(scatter_rows_kernel<uint32_t>, grid, dim3(256), 0, s, (uint32_t*)dst, (const uint32_t*)src, rows, m, w);
    return hipGetLastError();
}

// ---- watch lists: time series of chosen rows out of the telemetry ring ------------------------------------------
// Ring of component k: [ring][n, w_k] blocks in the reference row layout, tick t in slot history_slot(t).  The step kernel
// writes the four Body columns that way (step_kernel.hpp `record`), snapshot_tick_to_ring copies them that way, and a
// generated program's record() stores `(slot * P.n + row) * w + j` whatever layout its LIVE columns have (codegen.py
// `records`: element-major `column_soa` programs index only the source g0 differently) — so one kernel reads every ring.
// Output of component k: out[m][n_samples][w_k], one contiguous series per (row, component) pair, sample j = tick
// first_tick + j * every.
//
// Thread mapping: one thread per OUTPUT element, consecutive threads on consecutive elements, so every store instruction
// of a wave is one contiguous 256- or 512-byte run.  The loads of a wave fall into ceil(64 / w) pieces of w contiguous
// elements, n * w elements apart (neighbouring samples of one row): a gather of 24- to 56-byte rows that are each read
// once has nothing to stage or reuse, so no LDS; it is bounded by those pieces, and moves m * n_samples rows, not n.
// All index arithmetic is 64-bit: slot * n * w passes 2^32 at 65,536 rows and a few thousand slots.
template <class E>
__global__ __launch_bounds__(256) void history_gather_kernel(HistoryGatherArgs a, E* __restrict__ out,
                                                             const uint32_t* __restrict__ rows, uint64_t m, uint64_t n,
                                                             uint64_t first_tick, uint64_t n_samples, uint64_t every,
                                                             uint64_t ring) {
    const HistoryGatherDesc d = a.c[blockIdx.y];
    const E* __restrict__ src = static_cast<const E*>(d.ring);
    E* __restrict__ dst = out + d.out_offset;
    const uint64_t w = d.w, series = n_samples * w, total = m * series;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const uint64_t e = i / series, in_series = i - e * series;
        const uint64_t j = in_series / w, c = in_series - j * w;
        const uint64_t slot = sample_slot(first_tick, j, every, ring);
        dst[i] = src[(slot * n + rows[e]) * w + c];
    }
}

hipError_t launch_history_gather(const HistoryGatherArgs& a, uint32_t n_components, void* out, const uint32_t* rows,
                                 uint64_t m, uint64_t n, uint64_t first_tick, uint64_t n_samples, uint64_t every,
                                 uint64_t ring, size_t elem, hipStream_t s) {
    if (n_components == 0 || n_components > kHistoryGatherMax) return hipErrorInvalidValue;
    uint64_t w_max = 0;
    for (uint32_t k = 0; k < n_components; k++) w_max = a.c[k].w > w_max ? a.c[k].w : w_max;
    const uint64_t total = m * n_samples * w_max;
    if (total == 0) return hipSuccess;
    // the widest component sizes the grid (the others' spare threads find nothing to do); past 2^16 blocks a thread loops
    const uint64_t blocks = (total + 255) / 256;
    const dim3 grid((unsigned)(blocks < 65536 ? blocks : 65536), n_components);
    if (elem == 8) hipLaunchKernelGGL(history_gather_kernel<uint64_t>, grid, dim3(256), 0, s, a, (uint64_t*)out, rows, m, n, first_tick, n_samples, every, ring);
    else hipLaunchKernelGGL(history_gather_kernel<uint32_t>, grid, dim3(256), 0, s, a, (uint32_t*)out, rows, m, n, first_tick, n_samples, every, ring);
    return hipGetLastError();
}

// ---- failure sentinel: rows whose pose or velocity is no longer finite ------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void nonfinite_kernel(const T* __restrict__ pos, const T* __restrict__ vel, uint32_t n,
                                                        uint8_t* __restrict__ flags, unsigned long long* __restrict__ count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (i < n) {
        for (int c = 0; c < 7; c++) bad |= !isfinite(pos[(size_t)i * 7 + c]);
        for (int c = 0; c < 6; c++) bad |= !isfinite(vel[(size_t)i * 6 + c]);
        if (flags) flags[i] = bad ? 1 : 0;
    }
    const unsigned long long m = __ballot(bad);   // 64-lane wave: one atomic per wave
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(count, (unsigned long long)__popcll(m));
}

hipError_t launch_nonfinite(const void* pos, const void* vel, uint32_t n, size_t elem, uint8_t* flags,
                            unsigned long long* count, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const dim3 grid((n + 255) / 256);
    if (elem == 8) hipLaunchKernelGGL(nonfinite_kernel<double>, grid, dim3(256), 0, s, (const double*)pos, (const double*)vel, n, flags, count);
    else hipLaunchKernelGGL(nonfinite_kernel<float>, grid, dim3(256), 0, s, (const float*)pos, (const float*)vel, n, flags, count);
    return hipGetLastError();
}

}  // namespace sixdof
