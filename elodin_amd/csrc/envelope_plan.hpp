// envelope_plan.hpp — geometry and arithmetic of the ring envelopes: per sampled tick and component element, count / min / max /
// mean / m2 over the rows of one group (row % period).  Pure arithmetic, no HIP: envelope_partial_kernel and envelope_merge_kernel
// (envelope_kernels.hip) and the host twin (hip_fake.cpp) run the same functions in the same order, sixdof_history_envelope
// (sixdof_capi.cpp) sizes its buffers and refuses what is too wide with them, envelope_host_test.cpp checks them on the host.
//
// One tick of one component is a flat block of n * w elements; element i belongs to bin i % (period * w) = group * w + column.
// A tile is the largest multiple of the bin count that fits the threads of a block, so thread t of a block meets only bin
// t % bins, whichever tile it reads, while consecutive threads read consecutive elements.  Tile k goes to block k % blocks.
#pragma once

#include <cstdint>

#include "history_plan.hpp"

namespace sixdof {

constexpr uint32_t kEnvelopeThreads = 512;     // threads of a stage-1 block
constexpr uint32_t kEnvelopeMaxBins = 512;     // period * w a block can keep apart: one thread per bin at least
constexpr uint32_t kEnvelopeMaxBlocks = 32;    // stage-1 blocks per (sample, component)
constexpr uint32_t kEnvelopeTilesPerBlock = 4; // fewer blocks rather than blocks with less than this to read
constexpr uint32_t kEnvelopeStats = 5;         // count, min, max, mean, m2

// How the n * w elements of one tick are dealt out.  A pure function of (n, w, period): nothing else may enter, so that the
// value for one (tick, component) is bit-identical however it is read.
struct EnvelopeGeom {
    uint32_t bins;      // period * w
    uint32_t per_bin;   // threads of a block that share a bin
    uint32_t tile;      // bins * per_bin <= kEnvelopeThreads: elements a block reads at once
    uint32_t blocks;    // stage-1 blocks, each writes `bins` partial records
    uint64_t tiles;     // ceil(n * w / tile)
};
SIXDOF_HOST_DEVICE inline bool envelope_supported(uint64_t w, uint64_t period) {
    return w >= 1 && period >= 1 && period <= kEnvelopeMaxBins && w <= kEnvelopeMaxBins && period * w <= kEnvelopeMaxBins;
}
// What launch_history_envelope accepts, for the launcher (envelope_kernels.hip) and its host twin (hip_fake.cpp) alike: at most
// `max_components` (kernels.hpp: kRingBinMaxComponents) components, a grid y extent of n_samples below 2^16.
inline bool envelope_launch_ok(uint32_t n_components, uint32_t max_components, uint64_t n_samples, uint32_t period) {
    return n_components != 0 && n_components <= max_components && n_samples <= 65535 && period != 0;
}
SIXDOF_HOST_DEVICE inline EnvelopeGeom envelope_geom(uint64_t n, uint32_t w, uint32_t period) {
    EnvelopeGeom g{};
    g.bins = period * w;
    g.per_bin = kEnvelopeThreads / g.bins;
    g.tile = g.bins * g.per_bin;
    g.tiles = (n * w + g.tile - 1) / g.tile;
    const uint64_t want = (g.tiles + kEnvelopeTilesPerBlock - 1) / kEnvelopeTilesPerBlock;
    g.blocks = static_cast<uint32_t>(want < 1 ? 1 : want > kEnvelopeMaxBlocks ? kEnvelopeMaxBlocks : want);
    return g;
}

// A thread's running state, what stage 1 hands to stage 2, and what a merge combines.  count == 0: the identity (min = +inf,
// max = -inf).
struct EnvelopePartial {
    double count, min, max, mean, m2;
};
SIXDOF_HOST_DEVICE inline EnvelopePartial envelope_empty() { return {0.0, __builtin_inf(), -__builtin_inf(), 0.0, 0.0}; }

// Welford's update: against 6.4e6 m +- metres it keeps what the textbook sum of squares loses, and its error stays within the
// bound of the updating algorithms (Chan, Golub, LeVeque 1983) at every count — sums shifted by the first value met do not at
// counts of a few, where that value is far from the mean.  The division per element costs nothing a bandwidth-bound kernel
// would notice.  Non-finite values are skipped: a diverged run does not erase the envelope of the others.
SIXDOF_HOST_DEVICE inline void envelope_accumulate(EnvelopePartial& a, double x) {
    if (!__builtin_isfinite(x)) return;
    a.count += 1.0;
    const double delta = x - a.mean;
    a.mean += delta / a.count;
    a.m2 += delta * (x - a.mean);
    a.min = x < a.min ? x : a.min;
    a.max = x > a.max ? x : a.max;
}
// Chan's pairwise update; `a` is the left operand of every merge order below.
SIXDOF_HOST_DEVICE inline EnvelopePartial envelope_merge(const EnvelopePartial& a, const EnvelopePartial& b) {
    if (b.count == 0.0) return a;
    if (a.count == 0.0) return b;
    const double n = a.count + b.count, delta = b.mean - a.mean;
    EnvelopePartial r;
    r.count = n;
    r.min = b.min < a.min ? b.min : a.min;
    r.max = b.max > a.max ? b.max : a.max;
    r.mean = a.mean + delta * b.count / n;
    r.m2 = a.m2 + b.m2 + delta * delta * a.count * b.count / n;
    return r;
}

// Merge order inside a block: the per_bin records of one bin, record j held by thread j * bins + bin, fold as a binary tree
// — for s = envelope_tree_start(per_bin), s / 2, ... 1: record j < s takes record j + s where that exists.
SIXDOF_HOST_DEVICE inline uint32_t envelope_tree_start(uint32_t per_bin) {
    uint32_t s = 1;
    while (s * 2 < per_bin) s *= 2;
    return per_bin > 1 ? s : 0;
}
// Serial form of that tree over rec[j * stride], j < per_bin; the result is left in rec[0].
SIXDOF_HOST_DEVICE inline void envelope_tree_fold(EnvelopePartial* rec, uint32_t per_bin, uint32_t stride) {
    for (uint32_t s = envelope_tree_start(per_bin); s >= 1; s /= 2)
        for (uint32_t j = 0; j < s && j + s < per_bin; j++) rec[j * stride] = envelope_merge(rec[j * stride], rec[(j + s) * stride]);
}

// The five output values of one bin, [5][w] apart in the output block: count == 0 leaves the four statistics NaN.
SIXDOF_HOST_DEVICE inline void envelope_emit(const EnvelopePartial& p, double* out, uint64_t stat_stride) {
    const double nan = __builtin_nan("");
    const bool any = p.count != 0.0;
    out[0] = p.count;
    out[stat_stride] = any ? p.min : nan;
    out[2 * stat_stride] = any ? p.max : nan;
    out[3 * stat_stride] = any ? p.mean : nan;
    out[4 * stat_stride] = any ? p.m2 : nan;
}

}  // namespace sixdof
