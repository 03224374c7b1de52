// quantile_kernels.hip — ring quantiles: per sampled tick and component element, exact order statistics x(lo), x(hi) of rational
// ranks over the finite rows of one group (row % period), selected on the device so that 1 + 2 * ranks numbers per element and
// tick cross the link, not n rows.  Keys, rank arithmetic, the scan step and the lo -> hi rule are quantile_plan.hpp's, shared
// with the host twin.
//
// One tick of one component is n / period rows of bins = period * w columns, contiguous (element i in bin i % bins).  A radix
// select, most significant byte first: 8 passes for f64 keys, 4 for f32, and a closing pass for x(hi) — passes + 1 reads of a
// tick's block, which stays in L2 / the Infinity Cache between them: the blocks of one (sample, component) are neighbours in
// the grid (blockIdx.x).
//
// quantile_hist_kernel, grid (splits * row_blocks, samples, components): a block keeps the 256-counter histograms of all ranks
// of g.cols consecutive bins in LDS (48 KiB).  Thread t reads column t % cols of row t / cols of each sweep: where cols == bins
// (bins * ranks <= 48) that is the envelope's pattern, consecutive lanes on consecutive elements and a thread on one bin; wider
// bin counts are split into column ranges, a lane run then covers `cols` consecutive elements of every row.  Four loads per
// lane are in flight.  Ranks of a bin whose prefixes are equal count the same elements and share one histogram (all of them in
// pass 0), so an element costs one LDS atomic per DISTINCT matching prefix — about one in the early passes, none in the late
// ones, where most elements match no prefix.  Equal (histogram, digit) addresses of a wave are combined before the atomic (a
// column's values share their top bytes): ballot the lanes that want the first pending address, one add of their count.
// The block then adds its non-zero counters to the sample's histograms in global memory.  Integer atomics only: they commute,
// the result does not depend on any order.
// quantile_scan_kernel: one thread per (sample, component, bin, rank) scans the histogram of its alias and advances its slot.
// quantile_next_kernel: the closing read — for the slots whose x(hi) is not x(lo), the smallest key above x(lo), an integer min.
// quantile_emit_kernel: keys back to elements, converted to double, into the staging block.
// All index arithmetic is 64-bit.
#include <cstdlib>

#include "quantile_plan.hpp"
#include "kernels.hpp"

namespace sixdof {

// One (histogram, digit) counter more for every lane that is `on`.  ROUNDS > 0: up to that many distinct addresses of the wave
// are added once each, with the number of lanes that share them; what is left after that is added lane by lane.
template <int ROUNDS>
__device__ __forceinline__ void quantile_count(uint32_t* hist, bool on, uint32_t addr) {
    if constexpr (ROUNDS > 0) {
        const int lane = threadIdx.x & 63;
#pragma unroll 1
        for (int round = 0; round < ROUNDS; round++) {
            const uint64_t todo = __ballot(on);
            if (todo == 0) return;
            const int leader = __ffsll(static_cast<unsigned long long>(todo)) - 1;
            const uint32_t first = __shfl(addr, leader);
            const bool same = on && addr == first;
            const uint64_t group = __ballot(same);
            if (lane == leader) atomicAdd(&hist[first], static_cast<uint32_t>(__popcll(group)));
            on = on && !same;
        }
    }
    if (on) atomicAdd(&hist[addr], 1u);
}

// The rows dealt to row block `rb`, columns col0 .. col0 + cols - 1: f(valid, element) for every thread alike (the trip count is
// the block's, a thread without an element takes part with valid == false), four loads ahead.
template <class E, class F>
__device__ __forceinline__ void quantile_for_each(const E* __restrict__ src, const QuantileGeom& g, uint32_t col0, uint32_t cols, uint32_t rb, F&& f) {
    const uint32_t i = threadIdx.x % cols, j = threadIdx.x / cols;
    const bool mine = j < g.sweep;
    const uint64_t step = static_cast<uint64_t>(g.row_blocks) * g.sweep;
    for (uint64_t base = static_cast<uint64_t>(rb) * g.sweep; base < g.rows; base += 4 * step) {
        E x[4];
        bool valid[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint64_t row = base + u * step + j;
            valid[u] = mine && row < g.rows;
            x[u] = valid[u] ? src[row * g.bins + col0 + i] : E(0);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) f(valid[u], x[u]);
    }
}

struct QuantileBlock {
    uint32_t col0, cols, rb;
    uint64_t slot0;   // the block's first (bin, rank) slot in the launch's scratch
};
__device__ __forceinline__ bool quantile_block(const RingBinDesc& d, const QuantileGeom& g, uint32_t ranks, uint64_t slot_stride, QuantileBlock* b) {
    if (blockIdx.x >= g.splits * g.row_blocks) return false;   // a component with fewer blocks than the one that sized the grid
    const uint32_t split = blockIdx.x / g.row_blocks;
    b->rb = blockIdx.x % g.row_blocks;
    b->col0 = split * g.cols;
    b->cols = g.bins - b->col0 < g.cols ? g.bins - b->col0 : g.cols;
    b->slot0 = static_cast<uint64_t>(blockIdx.y) * slot_stride + d.scratch_offset + static_cast<uint64_t>(b->col0) * ranks;
    return true;
}

template <class E, int ROUNDS>
__global__ __launch_bounds__(kQuantileThreads) void quantile_hist_kernel(RingBinArgs a, uint32_t ranks, uint32_t* __restrict__ hist,
                                                                         const QuantileSlot* __restrict__ state, uint64_t slot_stride, uint64_t n,
                                                                         uint32_t period, uint32_t pass, uint64_t first_tick, uint64_t sample0,
                                                                         uint64_t every, uint64_t ring) {
    using B = QuantileBits<E>;
    __shared__ uint32_t s_hist[kQuantileBlockSlots * kQuantileDigits];
    __shared__ uint64_t s_prefix[kQuantileBlockSlots];   // of every slot of the block
    __shared__ uint64_t s_want[kQuantileBlockSlots];     // per column: its distinct prefixes, s_distinct[column] of them
    __shared__ uint32_t s_slot[kQuantileBlockSlots];     //             and the slot that counts each
    __shared__ uint32_t s_distinct[kQuantileBlockSlots];
    __shared__ uint32_t s_most;
    const RingBinDesc d = a.c[blockIdx.z];
    const QuantileGeom g = quantile_geom(n, d.w, period, ranks);
    QuantileBlock b;
    if (!quantile_block(d, g, ranks, slot_stride, &b)) return;
    const uint32_t t = threadIdx.x, slots = b.cols * ranks;
    for (uint32_t c = t; c < slots * kQuantileDigits; c += kQuantileThreads) s_hist[c] = 0;
    if (t == 0) s_most = 0;
    if (t < slots) s_prefix[t] = pass == 0 ? 0 : state[b.slot0 + t].prefix;
    __syncthreads();
    if (t < b.cols) {
        uint32_t distinct = 0;
        if (pass == 0 || !(state[b.slot0 + t * ranks].flags & kQuantileEmpty))
            for (uint32_t r = 0; r < ranks; r++)
                if (quantile_alias(&s_prefix[t * ranks], r) == r) {
                    s_want[t * ranks + distinct] = s_prefix[t * ranks + r];
                    s_slot[t * ranks + distinct] = t * ranks + r;
                    distinct++;
                }
        s_distinct[t] = distinct;
        atomicMax(&s_most, distinct);
    }
    __syncthreads();
    const uint64_t total = n * d.w;
    const E* __restrict__ src = static_cast<const E*>(d.ring) + sample_slot(first_tick, sample0 + blockIdx.y, every, ring) * total;
    const uint32_t mine = (t % b.cols) * ranks, distinct = s_distinct[t % b.cols], most = s_most;
    const uint32_t shift = quantile_shift(B::bits, pass);
    const uint64_t mask = quantile_prefix_mask(B::bits, pass);
    quantile_for_each(src, g, b.col0, b.cols, b.rb, [&](bool valid, E x) {
        const uint64_t u = B::raw(x), key = B::key(u), high = key & mask;
        const uint32_t digit = quantile_digit(key, shift);
        valid = valid && B::finite(u);
        for (uint32_t q = 0; q < most; q++) {
            const bool on = valid && q < distinct && high == s_want[mine + q];
            quantile_count<ROUNDS>(s_hist, on, on ? s_slot[mine + q] * kQuantileDigits + digit : 0u);
        }
    });
    __syncthreads();
    uint32_t* __restrict__ to = hist + b.slot0 * kQuantileDigits;
    for (uint32_t c = t; c < slots * kQuantileDigits; c += kQuantileThreads)
        if (const uint32_t v = s_hist[c]) atomicAdd(&to[c], v);
}

// 16 bins x 16 ranks per block: the ranks of a bin see each other's prefixes as they were before this pass.
template <class E>
__global__ __launch_bounds__(256) void quantile_scan_kernel(RingBinArgs a, QuantileRanks ranks, const uint32_t* __restrict__ hist,
                                                            QuantileSlot* __restrict__ state, uint64_t slot_stride, uint64_t n, uint32_t period,
                                                            uint32_t pass) {
    __shared__ uint64_t s_old[16][kQuantileMaxRanks];
    const RingBinDesc d = a.c[blockIdx.z];
    const uint32_t bins = envelope_geom(n, d.w, period).bins;
    const uint32_t r = threadIdx.x % kQuantileMaxRanks, local = threadIdx.x / kQuantileMaxRanks, bin = blockIdx.x * 16 + local;
    const bool mine = bin < bins && r < ranks.count;
    const uint64_t slot0 = static_cast<uint64_t>(blockIdx.y) * slot_stride + d.scratch_offset + static_cast<uint64_t>(bin) * ranks.count;
    QuantileSlot s{};
    if (mine && pass > 0) s = state[slot0 + r];
    s_old[local][r] = s.prefix;
    __syncthreads();
    if (!mine) return;
    const uint32_t alias = quantile_alias(s_old[local], r);
    uint32_t num = 0;
#pragma unroll
    for (uint32_t q = 0; q < kQuantileMaxRanks; q++) num = q == r ? ranks.num[q] : num;
    quantile_advance(s, hist + (slot0 + alias) * kQuantileDigits, QuantileBits<E>::bits, pass, num, ranks.den);
    state[slot0 + r] = s;
}

constexpr uint64_t kQuantileNoKey = ~uint64_t(0);   // above every finite key: what the cleared (all ones) scratch reads as

template <class E>
__global__ __launch_bounds__(kQuantileThreads) void quantile_next_kernel(RingBinArgs a, uint32_t ranks, uint64_t* __restrict__ next,
                                                                         const QuantileSlot* __restrict__ state, uint64_t slot_stride, uint64_t n,
                                                                         uint32_t period, uint64_t first_tick, uint64_t sample0, uint64_t every,
                                                                         uint64_t ring) {
    using B = QuantileBits<E>;
    __shared__ uint64_t s_above[kQuantileBlockSlots];   // the key of x(lo), or no key where x(hi) needs no search
    __shared__ uint64_t s_min[kQuantileBlockSlots];
    const RingBinDesc d = a.c[blockIdx.z];
    const QuantileGeom g = quantile_geom(n, d.w, period, ranks);
    QuantileBlock b;
    if (!quantile_block(d, g, ranks, slot_stride, &b)) return;
    const uint32_t t = threadIdx.x, slots = b.cols * ranks;
    if (t < slots) {
        const QuantileSlot s = state[b.slot0 + t];
        s_above[t] = (s.flags & kQuantileNeedNext) ? s.prefix : kQuantileNoKey;
        s_min[t] = kQuantileNoKey;
    }
    __syncthreads();
    const uint64_t total = n * d.w;
    const E* __restrict__ src = static_cast<const E*>(d.ring) + sample_slot(first_tick, sample0 + blockIdx.y, every, ring) * total;
    const uint32_t mine = (t % b.cols) * ranks;
    quantile_for_each(src, g, b.col0, b.cols, b.rb, [&](bool valid, E x) {
        const uint64_t u = B::raw(x), key = B::key(u);
        if (!valid || !B::finite(u)) return;
        for (uint32_t r = 0; r < ranks; r++)   // the running minimum is read first: soon almost nothing gets to the atomic
            if (key > s_above[mine + r] && key < __hip_atomic_load(&s_min[mine + r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
                atomicMin(reinterpret_cast<unsigned long long*>(&s_min[mine + r]), static_cast<unsigned long long>(key));
    });
    __syncthreads();
    if (t < slots && s_min[t] != kQuantileNoKey)
        atomicMin(reinterpret_cast<unsigned long long*>(&next[(b.slot0 + t) * (kQuantileDigits / 2)]), static_cast<unsigned long long>(s_min[t]));
}

template <class E>
__global__ __launch_bounds__(256) void quantile_emit_kernel(RingBinArgs a, uint32_t ranks, const uint64_t* __restrict__ next,
                                                            const QuantileSlot* __restrict__ state, uint64_t slot_stride, double* __restrict__ out,
                                                            uint64_t n, uint32_t period, uint64_t sample0) {
    const RingBinDesc d = a.c[blockIdx.z];
    const uint32_t bins = envelope_geom(n, d.w, period).bins;
    const uint32_t r = threadIdx.x % kQuantileMaxRanks, bin = blockIdx.x * 16 + threadIdx.x / kQuantileMaxRanks;
    if (bin >= bins || r >= ranks) return;
    const uint64_t slot = static_cast<uint64_t>(blockIdx.y) * slot_stride + d.scratch_offset + static_cast<uint64_t>(bin) * ranks + r;
    const uint64_t group = bin / d.w, c = bin % d.w, sample = sample0 + blockIdx.y, planes = 1 + 2 * static_cast<uint64_t>(ranks);
    quantile_emit<E>(state[slot], next[slot * (kQuantileDigits / 2)], r, out + d.out_offset + ((sample * period + group) * planes) * d.w + c, d.w);
}

// Distinct addresses of a wave combined before the LDS atomic: 8 rounds by default; SIXDOF_QUANTILE_ROUNDS = 0 (every lane its
// own atomic) or 64 (every address once) select the other forms for A/B runs (tools/history_quantiles_ab.py).
static int quantile_rounds() {
    static const int rounds = [] {
        const char* e = std::getenv("SIXDOF_QUANTILE_ROUNDS");
        return e ? std::atoi(e) : 8;
    }();
    return rounds;
}

template <class E>
static hipError_t quantile_launches(const RingBinArgs& a, uint32_t n_components, const QuantileRanks& ranks, double* out, uint32_t* hist,
                                    QuantileSlot* state, uint64_t slot_stride, uint64_t n, uint32_t period, uint64_t first_tick,
                                    uint64_t sample0, uint64_t n_samples, uint64_t every, uint64_t ring, uint32_t blocks, uint32_t bins,
                                    hipStream_t s) {
    const dim3 grid(blocks, (unsigned)n_samples, n_components), per_slot((bins + 15) / 16, (unsigned)n_samples, n_components);
    const size_t hist_bytes = static_cast<size_t>(n_samples) * slot_stride * kQuantileDigits * sizeof(uint32_t);
    const int rounds = quantile_rounds();
    for (uint32_t pass = 0; pass < quantile_passes(QuantileBits<E>::bits); pass++) {
        if (hipError_t e = hipMemsetAsync(hist, 0, hist_bytes, s); e != hipSuccess) return e;
        auto kernel = rounds == 0 ? quantile_hist_kernel<E, 0> : rounds >= 64 ? quantile_hist_kernel<E, 64> : quantile_hist_kernel<E, 8>;
        hipLaunchKernelGGL(kernel, grid, dim3(kQuantileThreads), 0, s, a, ranks.count, hist, state, slot_stride, n, period, pass, first_tick, sample0, every, ring);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        hipLaunchKernelGGL(quantile_scan_kernel<E>, per_slot, dim3(256), 0, s, a, ranks, hist, state, slot_stride, n, period, pass);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    uint64_t* next = reinterpret_cast<uint64_t*>(hist);   // the first 8 bytes of a slot's histogram: all ones is "no key"
    if (hipError_t e = hipMemsetAsync(hist, 0xff, hist_bytes, s); e != hipSuccess) return e;
    hipLaunchKernelGGL(quantile_next_kernel<E>, grid, dim3(kQuantileThreads), 0, s, a, ranks.count, next, state, slot_stride, n, period, first_tick, sample0, every, ring);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(quantile_emit_kernel<E>, per_slot, dim3(256), 0, s, a, ranks.count, next, state, slot_stride, out, n, period, sample0);
    return hipGetLastError();
}

hipError_t launch_history_quantiles(const RingBinArgs& a, uint32_t n_components, const QuantileRanks& ranks, double* out, void* hist,
                                    void* state, uint64_t slot_stride, uint64_t n, uint32_t period, uint64_t first_tick,
                                    uint64_t sample0, uint64_t n_samples, uint64_t every, uint64_t ring, size_t elem, hipStream_t s) {
    if (!quantile_launch_ok(n_components, kRingBinMaxComponents, ranks, n, n_samples, period)) return hipErrorInvalidValue;
    if (n_samples == 0 || n == 0) return hipSuccess;
    uint32_t blocks = 0, bins = 0;
    for (uint32_t k = 0; k < n_components; k++) {
        if (!envelope_supported(a.c[k].w, period)) return hipErrorInvalidValue;
        const QuantileGeom g = quantile_geom(n, a.c[k].w, period, ranks.count);
        blocks = g.splits * g.row_blocks > blocks ? g.splits * g.row_blocks : blocks;
        bins = g.bins > bins ? g.bins : bins;
    }
    uint32_t* h = static_cast<uint32_t*>(hist);
    QuantileSlot* st = static_cast<QuantileSlot*>(state);
    return elem == 8 ? quantile_launches<double>(a, n_components, ranks, out, h, st, slot_stride, n, period, first_tick, sample0, n_samples, every, ring, blocks, bins, s)
                     : quantile_launches<float>(a, n_components, ranks, out, h, st, slot_stride, n, period, first_tick, sample0, n_samples, every, ring, blocks, bins, s);
}

}  // namespace sixdof
