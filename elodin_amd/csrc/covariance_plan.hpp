// covariance_plan.hpp — geometry and arithmetic of the ring covariances: per sampled tick and group (row % period), the count,
// the mean vector and the upper triangle of the co-moment matrix C[a][b] = sum (x_a - mean_a)(x_b - mean_b) of k channels, a
// channel being one element of one recorded component.  Pure arithmetic, no HIP: covariance_partial_kernel and
// covariance_merge_kernel (covariance_kernels.hip) and the host twin (hip_fake.cpp) run the same functions in the same order,
// sixdof_history_covariance (sixdof_capi.cpp) sizes its buffers and refuses with them, covariance_host_test.cpp checks them.
//
// One thread per ROW, not per element: a row's k values meet in one thread, so a row is used or skipped as a whole.  A tile is the
// largest multiple of `period` that fits the threads of a block, so thread t stays on group t % period whichever tile it reads,
// while consecutive threads read consecutive rows.  Tile i goes to block i % blocks.
//
// Rounding: every function here is compiled WITHOUT contraction of a multiply and an add into an FMA (the pragma below for clang,
// which overrides kernels.hpp's file-wide "on"; g++ builds of the host twin pass -ffp-contract=off), so the kernels, the twin and
// a test's serial restatement round alike, bit for bit.
#pragma once

#include <cstdint>

#include "envelope_plan.hpp"

#if defined(__clang__)
#define SIXDOF_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define SIXDOF_NO_CONTRACT
#endif

namespace sixdof {

constexpr uint32_t kCovarianceMaxChannels = 6;     // a body's position plus velocity
#ifndef SIXDOF_COVARIANCE_THREADS
#define SIXDOF_COVARIANCE_THREADS 256
#endif
#ifndef SIXDOF_COVARIANCE_MAX_BLOCKS
#define SIXDOF_COVARIANCE_MAX_BLOCKS 8
#endif
// Threads of a stage-1 block and the cap on stage-1 blocks per sample: chosen from the "threads of a stage-1 block x cap on blocks
// per sample" tables of profiles/history_covariance.md (tools/history_covariance_ab.py; `make cov_variant` builds the other cells
// through the two macros above).  At 6 channels a record is 224 bytes: 256 of them are 56 KB of LDS, two blocks per CU; 512 are
// 112 KB of the CU's 160 KB, one, and measured slower.  A block ends in a tree of log2(256) merges of whole records and writes
// `period` of them, which is what more blocks per sample cost: over 1,024 samples of 65,536 rows a cap of 8 beats 32 and 128.
constexpr uint32_t kCovarianceThreads = SIXDOF_COVARIANCE_THREADS;
constexpr uint32_t kCovarianceMaxBlocks = SIXDOF_COVARIANCE_MAX_BLOCKS;
constexpr uint32_t kCovarianceMaxPeriod = kCovarianceThreads;   // groups a block can keep apart: one thread per group at least
constexpr uint32_t kCovarianceTilesPerBlock = 4;   // fewer blocks rather than blocks with less than this to read
constexpr uint32_t kCovarianceRowsInFlight = 4;    // rows whose k loads a lane issues before it consumes the first

constexpr uint32_t covariance_fields(uint32_t k) { return 1 + k + k * (k + 1) / 2; }   // doubles of a record and of an output entry
constexpr uint32_t covariance_pair(uint32_t k, uint32_t a, uint32_t b) { return a * k - a * (a + 1) / 2 + b; }   // a <= b: row-major upper triangle
constexpr size_t kCovarianceLdsLimit = 160 * 1024;   // LDS of a gfx950 CU
constexpr size_t covariance_lds_bytes(uint32_t k) { return size_t(kCovarianceThreads) * covariance_fields(k) * sizeof(double); }
static_assert(covariance_lds_bytes(2) <= kCovarianceLdsLimit && covariance_lds_bytes(3) <= kCovarianceLdsLimit && covariance_lds_bytes(4) <= kCovarianceLdsLimit &&
                  covariance_lds_bytes(5) <= kCovarianceLdsLimit && covariance_lds_bytes(6) <= kCovarianceLdsLimit,
              "a stage-1 block's records do not fit the LDS of a CU");

SIXDOF_HOST_DEVICE inline bool covariance_supported(uint64_t k, uint64_t period) {
    return k >= 2 && k <= kCovarianceMaxChannels && period >= 1 && period <= kCovarianceMaxPeriod;
}

// How the n rows of one tick are dealt out.  A pure function of (n, period): nothing else may enter — not the channels, the
// range, `every`, the flags or the chunk — so that the value for one (tick, channel list, period) is bit-identical however it
// is read.
struct CovarianceGeom {
    uint32_t per_group;   // threads of a block that share a group
    uint32_t tile;        // period * per_group <= kCovarianceThreads: rows a block reads at once
    uint32_t blocks;      // stage-1 blocks, each writes `period` partial records
    uint64_t tiles;       // ceil(n / tile)
};
SIXDOF_HOST_DEVICE inline CovarianceGeom covariance_geom(uint64_t n, uint32_t period) {
    CovarianceGeom g{};
    g.per_group = kCovarianceThreads / period;
    g.tile = period * g.per_group;
    g.tiles = (n + g.tile - 1) / g.tile;
    const uint64_t want = (g.tiles + kCovarianceTilesPerBlock - 1) / kCovarianceTilesPerBlock;
    g.blocks = static_cast<uint32_t>(want < 1 ? 1 : want > kCovarianceMaxBlocks ? kCovarianceMaxBlocks : want);
    return g;
}
// Scratch of one sample: [blocks][fields][period] doubles — field-major, so that the `period` threads that write or read one
// field of one block touch consecutive doubles.
SIXDOF_HOST_DEVICE inline uint64_t covariance_scratch_doubles(const CovarianceGeom& g, uint32_t k, uint32_t period) {
    return uint64_t(g.blocks) * covariance_fields(k) * period;
}
// What launch_history_covariance accepts, for the launcher and its host twin alike: a grid y extent of n_samples below 2^16.
inline bool covariance_launch_ok(uint32_t k, uint64_t n_samples, uint32_t period) { return covariance_supported(k, period) && n_samples <= 65535; }

// A thread's running state, what stage 1 hands to stage 2, and what a merge combines.  count == 0 (all zero): the identity.
template <int K>
struct CovarianceRecord {
    double count;
    double mean[K];
    double c[K * (K + 1) / 2];   // C[a][b], a <= b, at covariance_pair(K, a, b)
};
template <int K>
SIXDOF_HOST_DEVICE inline CovarianceRecord<K> covariance_empty() { return CovarianceRecord<K>{}; }

// Field f of a record, f < covariance_fields(K): count, the means, the triangle.  With f a compile-time constant after
// unrolling this is a register, not an indexed array.
template <int K>
SIXDOF_HOST_DEVICE inline double& covariance_field(CovarianceRecord<K>& r, int f) { return f == 0 ? r.count : f <= K ? r.mean[f - 1] : r.c[f - 1 - K]; }
template <int K>
SIXDOF_HOST_DEVICE inline double covariance_field(const CovarianceRecord<K>& r, int f) { return f == 0 ? r.count : f <= K ? r.mean[f - 1] : r.c[f - 1 - K]; }

// One row.  Listwise: the row counts only if all K values are finite — otherwise it is skipped for every mean and every
// co-moment, so that the matrix stays that of ONE population.  The multivariate form of Welford's update (envelope_plan.hpp
// says why not sums of products): the old means give d, the new means the second factor.
template <int K>
SIXDOF_HOST_DEVICE inline void covariance_accumulate(CovarianceRecord<K>& r, const double (&x)[K]) {
    SIXDOF_NO_CONTRACT
    bool finite = true;
    for (int a = 0; a < K; a++) finite = finite && __builtin_isfinite(x[a]);
    if (!finite) return;
    r.count += 1.0;
    double d[K], e[K];
    for (int a = 0; a < K; a++) d[a] = x[a] - r.mean[a];
    for (int a = 0; a < K; a++) {
        r.mean[a] += d[a] / r.count;
        e[a] = x[a] - r.mean[a];
    }
    for (int a = 0, i = 0; a < K; a++)
        for (int b = a; b < K; b++, i++) {
            const double term = d[a] * e[b];
            r.c[i] += term;
        }
}
// Chan's pairwise update, as generalised to co-moments by Pébay; `a` is the left operand of every merge order below.
template <int K>
SIXDOF_HOST_DEVICE inline CovarianceRecord<K> covariance_merge(const CovarianceRecord<K>& a, const CovarianceRecord<K>& b) {
    SIXDOF_NO_CONTRACT
    if (b.count == 0.0) return a;
    if (a.count == 0.0) return b;
    const double n = a.count + b.count;
    double delta[K];
    CovarianceRecord<K> r;
    r.count = n;
    for (int i = 0; i < K; i++) {
        delta[i] = b.mean[i] - a.mean[i];
        const double shift = delta[i] * b.count / n;
        r.mean[i] = a.mean[i] + shift;
    }
    for (int i = 0, p = 0; i < K; i++)
        for (int j = i; j < K; j++, p++) {
            const double cross = delta[i] * delta[j] * a.count * b.count / n;
            const double both = a.c[p] + b.c[p];
            r.c[p] = both + cross;
        }
    return r;
}

// Merge order inside a block: the per_group records of one group, record j held by thread j * period + group, fold as the
// binary tree of envelope_tree_start(per_group).  Serial form over rec[j * stride], j < per_group; the result is left in rec[0].
template <int K>
SIXDOF_HOST_DEVICE inline void covariance_tree_fold(CovarianceRecord<K>* rec, uint32_t per_group, uint32_t stride) {
    for (uint32_t s = envelope_tree_start(per_group); s >= 1; s /= 2)
        for (uint32_t j = 0; j < s && j + s < per_group; j++) rec[j * stride] = covariance_merge(rec[j * stride], rec[(j + s) * stride]);
}

// The 1 + K + K (K + 1) / 2 output values of one (sample, group), contiguous: count == 0 leaves everything behind the count NaN.
template <int K>
SIXDOF_HOST_DEVICE inline void covariance_emit(const CovarianceRecord<K>& r, double* out) {
    const double nan = __builtin_nan("");
    const bool any = r.count != 0.0;
    out[0] = r.count;
    for (int f = 1; f < (int)covariance_fields(K); f++) out[f] = any ? covariance_field(r, f) : nan;
}

}  // namespace sixdof
