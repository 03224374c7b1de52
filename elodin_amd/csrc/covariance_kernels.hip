// covariance_kernels.hip — ring covariances: per sampled tick and group (row % period), count, mean vector and co-moment matrix
// of k channels (element e_a of recorded component c_a) across the rows, reduced on the device so that 1 + k + k (k + 1) / 2
// doubles per group and tick cross the link, not n rows of every touched component.
//
// Ring of a component: [ring][n, w] blocks in the reference row layout.  Geometry, accumulation and merge order are
// covariance_plan.hpp's, shared with the host twin; its functions are compiled without FMA contraction.
//
// Stage 1, covariance_partial_kernel<E, K>: grid (blocks, samples).  Thread t of a block takes row tile * g.tile + t of the tiles
// dealt to its block and gathers the row's K values: consecutive lanes read consecutive rows, so a wave's load of one channel
// spans 64 rows of w elements (a stride of w elements between lanes — every line of the touched columns is fetched once and
// shared by the channels of that component through L1 / L2).  kCovarianceRowsInFlight rows' loads are issued before the first
// is consumed.  Because g.tile is a multiple of the period the thread stays on group t % period and keeps one record in
// registers: K is a template parameter, so the record is never indexed at run time and nothing goes to scratch memory.  LDS
// only combines the per_group threads that share a group, as a binary tree in a fixed order; records lie field-major
// ([field][thread]) there, so a wave's access to one field is conflict-free.  Each block writes `period` records; no atomics.
// Stage 2, covariance_merge_kernel<K>: one thread per (sample, group) merges the records of blocks 0, 1, 2, ... in that order
// and writes the output entry.
// All index arithmetic is 64-bit: slot * n * w passes 2^32 at 65,536 rows and a few thousand slots.
#include "covariance_plan.hpp"
#include "kernels.hpp"

namespace sixdof {

template <int K>
__device__ inline void lds_put(double* lds, uint32_t t, const CovarianceRecord<K>& r) {
#pragma unroll
    for (int f = 0; f < (int)covariance_fields(K); f++) lds[f * kCovarianceThreads + t] = covariance_field(r, f);
}
template <int K>
__device__ inline CovarianceRecord<K> lds_get(const double* lds, uint32_t t) {
    CovarianceRecord<K> r;
#pragma unroll
    for (int f = 0; f < (int)covariance_fields(K); f++) covariance_field(r, f) = lds[f * kCovarianceThreads + t];
    return r;
}

template <class E, int K>
__global__ __launch_bounds__(kCovarianceThreads) void covariance_partial_kernel(CovarianceArgs a, double* __restrict__ partial, uint64_t partial_stride,
                                                                                uint64_t n, uint32_t period, uint64_t first_tick, uint64_t sample0,
                                                                                uint64_t every, uint64_t ring) {
    __shared__ double lds[covariance_fields(K) * kCovarianceThreads];
    const CovarianceGeom g = covariance_geom(n, period);
    const uint32_t b = blockIdx.x, t = threadIdx.x;
    const uint64_t slot = sample_slot(first_tick, sample0 + blockIdx.y, every, ring);
    const E* __restrict__ src[K];
    uint64_t w[K];
#pragma unroll
    for (int c = 0; c < K; c++) {
        w[c] = a.c[c].w;
        src[c] = static_cast<const E*>(a.c[c].ring) + slot * n * w[c] + a.c[c].element;
    }
    CovarianceRecord<K> acc = covariance_empty<K>();
    if (t < g.tile) {
        constexpr int R = kCovarianceRowsInFlight;
        const uint64_t step = (uint64_t)g.blocks * g.tile;
        uint64_t row = (uint64_t)b * g.tile + t;
        for (; row + (R - 1) * step < n; row += R * step) {
            E x[R][K];
#pragma unroll
            for (int i = 0; i < R; i++)
#pragma unroll
                for (int c = 0; c < K; c++) x[i][c] = src[c][(row + i * step) * w[c]];
#pragma unroll
            for (int i = 0; i < R; i++) {
                double v[K];
#pragma unroll
                for (int c = 0; c < K; c++) v[c] = (double)x[i][c];
                covariance_accumulate<K>(acc, v);
            }
        }
        for (; row < n; row += step) {
            double v[K];
#pragma unroll
            for (int c = 0; c < K; c++) v[c] = (double)src[c][row * w[c]];
            covariance_accumulate<K>(acc, v);
        }
    }
    lds_put<K>(lds, t, acc);
    __syncthreads();
    const uint32_t j = t / period;   // the t >= g.tile threads hold empty records and j >= per_group: they only meet the barriers
    for (uint32_t s = envelope_tree_start(g.per_group); s >= 1; s /= 2) {
        if (j < s && j + s < g.per_group) {
            acc = covariance_merge<K>(acc, lds_get<K>(lds, t + s * period));
            lds_put<K>(lds, t, acc);
        }
        __syncthreads();
    }
    if (t < period) {
        double* __restrict__ to = partial + (uint64_t)blockIdx.y * partial_stride + (uint64_t)b * covariance_fields(K) * period + t;
#pragma unroll
        for (int f = 0; f < (int)covariance_fields(K); f++) to[(uint64_t)f * period] = covariance_field(acc, f);
    }
}

template <int K>
__global__ __launch_bounds__(64) void covariance_merge_kernel(const double* __restrict__ partial, uint64_t partial_stride, double* __restrict__ out,
                                                              uint64_t n, uint32_t period, uint64_t sample0) {
    const CovarianceGeom g = covariance_geom(n, period);
    const uint32_t group = blockIdx.x * blockDim.x + threadIdx.x;
    if (group >= period) return;
    const double* __restrict__ p = partial + (uint64_t)blockIdx.y * partial_stride + group;
    CovarianceRecord<K> r = covariance_empty<K>();
    for (uint32_t b = 0; b < g.blocks; b++) {
        CovarianceRecord<K> o;
#pragma unroll
        for (int f = 0; f < (int)covariance_fields(K); f++) covariance_field(o, f) = p[((uint64_t)b * covariance_fields(K) + f) * period];
        r = b == 0 ? o : covariance_merge<K>(r, o);
    }
    covariance_emit<K>(r, out + ((sample0 + blockIdx.y) * period + group) * covariance_fields(K));
}

template <int K>
static hipError_t launch_k(const CovarianceArgs& a, double* out, double* partial, uint64_t partial_stride, uint64_t n, uint32_t period, uint64_t first_tick,
                           uint64_t sample0, uint64_t n_samples, uint64_t every, uint64_t ring, size_t elem, hipStream_t s) {
    const CovarianceGeom g = covariance_geom(n, period);
    const dim3 grid1(g.blocks, (unsigned)n_samples), grid2((period + 63) / 64, (unsigned)n_samples);
    if (elem == 8) hipLaunchKernelGGL((covariance_partial_kernel<double, K>), grid1, dim3(kCovarianceThreads), 0, s, a, partial, partial_stride, n, period, first_tick, sample0, every, ring);
    else hipLaunchKernelGGL((covariance_partial_kernel<float, K>), grid1, dim3(kCovarianceThreads), 0, s, a, partial, partial_stride, n, period, first_tick, sample0, every, ring);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(covariance_merge_kernel<K>, grid2, dim3(64), 0, s, partial, partial_stride, out, n, period, sample0);
    return hipGetLastError();
}

hipError_t launch_history_covariance(const CovarianceArgs& a, uint32_t k, double* out, void* partial, uint64_t partial_stride, uint64_t n, uint32_t period,
                                     uint64_t first_tick, uint64_t sample0, uint64_t n_samples, uint64_t every, uint64_t ring, size_t elem, hipStream_t s) {
    if (!covariance_launch_ok(k, n_samples, period)) return hipErrorInvalidValue;
    if (n_samples == 0 || n == 0) return hipSuccess;
    double* p = static_cast<double*>(partial);
    switch (k) {
    case 2: return launch_k<2>(a, out, p, partial_stride, n, period, first_tick, sample0, n_samples, every, ring, elem, s);
    case 3: return launch_k<3>(a, out, p, partial_stride, n, period, first_tick, sample0, n_samples, every, ring, elem, s);
    case 4: return launch_k<4>(a, out, p, partial_stride, n, period, first_tick, sample0, n_samples, every, ring, elem, s);
    case 5: return launch_k<5>(a, out, p, partial_stride, n, period, first_tick, sample0, n_samples, every, ring, elem, s);
    default: return launch_k<6>(a, out, p, partial_stride, n, period, first_tick, sample0, n_samples, every, ring, elem, s);
    }
}

}  // namespace sixdof
