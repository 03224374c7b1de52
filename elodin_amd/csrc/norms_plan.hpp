// norms_plan.hpp — the value, the walk and the geometry of the ring norms: per probe and run, over the sampled ticks of a range,
// the extremes of a SQUARED Euclidean norm — of 1 to 4 consecutive elements of one row, or of their difference to as many elements
// of another row of the same run — with the earliest sampled tick that holds each, the count of finite samples and the earliest
// tick at which the norm is not finite.  The kernels (norms_kernels.hip) and the host twin (hip_fake.cpp) run the same functions
// — norms_value, norms_walk and, for the rule, extremes_plan.hpp's extremes_accumulate and extremes_merge unchanged — and
// sixdof_history_norms (sixdof_capi.cpp) sizes its scratch with the geometry below; norms_host_test.cpp checks all of it on the host.
//
// A run is `period` consecutive rows.  Probe values are formed in f64 in one fixed order, every ring element widened first (exact
// for f32), without FMA contraction (SIXDOF_NO_CONTRACT on the device, -ffp-contract=off for the host twin): d_e = a_e or
// a_e - b_e, s = d_0 * d_0, then s = s + d_e * d_e for e = 1 .. count - 1.  So kernel, twin and a numpy restatement round alike,
// bit for bit.  A sample is finite exactly when s is: squares are non-negative, nothing cancels, any non-finite input gives a
// non-finite s — and so does an s that overflows from finite inputs.  s goes to the rule on QuantileBits<double> keys; a square
// is never -0.0.  The record, the six planes (extremes_emit<double> and extremes_absorb<double> are exact inverses: the values are
// doubles on either handle type), the scratch layout and the cut into time segments are extremes_plan.hpp's and time_scan.hpp's.
#pragma once

#include <cstddef>
#include <cstdint>

#include "covariance_plan.hpp"
#include "extremes_plan.hpp"

namespace sixdof {

constexpr uint32_t kNormsThreads = 256;         // threads of a block, one run each
constexpr uint32_t kNormsPlanes = kExtremesPlanes;   // SIXDOF_NORMS_PLANES: count, min_sq, tick_min, max_sq, tick_max, first_nonfinite
constexpr uint32_t kNormsFields = kExtremesFields;   // 64-bit fields of a record in scratch
constexpr uint32_t kNormsMaxProbes = 8;         // SIXDOF_NORMS_MAX_PROBES
constexpr uint32_t kNormsMaxCount = 4;          // SIXDOF_NORM_MAX_COUNT: a quaternion
constexpr uint32_t kNormMinus = 1;              // SIXDOF_NORM_MINUS
constexpr uint32_t kNormsMaxLoads = 16;         // ring elements a thread loads before it uses the first: see norms_depth
// Threads below which the plan cuts the samples (norms_segments).  Not derivable: it started from the events' 16,384 — the lanes
// are period * w elements apart there too — and the forced-segment table of profiles/history_norms.md (one |v| probe, 1,024
// ticks, reduced only, one MI355X) confirms that value for this walk: at 1,024 runs 0.247 ms in one segment, 0.134 in 2, 0.077 in
// 4, 0.051 in 8, 0.039 in 16 and 0.042 in 32; at 65,536 runs 1.031 ms in one, 1.044 in 2, 1.053 in 4, 1.080 in 8, 1.125 in 16 and
// 1.147 in 32.  So the rule picks 16 at 1,024 runs (the table's minimum) and 1 at 65,536.  Sizes between the two, and the chain
// length, have not been measured.
constexpr uint64_t kNormsFillThreads = 16384;

// One probe as the kernels see it: A is elements element_a .. element_a + count - 1 of row run * period + group_a of the
// component whose ring is ring_a; B likewise, read only with kNormMinus.
struct NormsProbe {
    const void* ring_a;   // [ring][n, w_a] blocks
    const void* ring_b;
    uint32_t w_a, w_b, element_a, element_b, group_a, group_b, count, flags;
};
struct NormsArgs { NormsProbe p[kNormsMaxProbes]; };   // by value: 384 bytes of kernel arguments

// ---- the value ------------------------------------------------------------------------------------------------------------
// The squared norm of one sample, in the order the header states.  `xb` is not read without MINUS.
template <class E, uint32_t COUNT, bool MINUS>
SIXDOF_HOST_DEVICE inline double norms_value(const E* xa, const E* xb) {
    SIXDOF_NO_CONTRACT
    double s = 0.0;
#pragma unroll
    for (uint32_t e = 0; e < COUNT; e++) {
        double d = static_cast<double>(xa[e]);
        if (MINUS) d = d - static_cast<double>(xb[e]);
        const double sq = d * d;
        s = e == 0 ? sq : s + sq;
    }
    return s;
}
// One sample, later than every sample `rec` has met: the rule applied to the derived scalar.
SIXDOF_HOST_DEVICE inline void norms_sample(ExtremesRecord& rec, double s, uint64_t tick) {
    const uint64_t u = QuantileBits<double>::raw(s);
    extremes_accumulate(rec, QuantileBits<double>::key(u), tick, QuantileBits<double>::finite(u));
}

// ---- the walk -------------------------------------------------------------------------------------------------------------
// Samples a thread loads before it uses the first.  A sample is COUNT independent loads, twice that with MINUS; scan_walk keeps
// kScanLoads = 4 single loads in flight.  Here the depth is what keeps at most kNormsMaxLoads = 16 elements (32 VGPRs of f64)
// in flight, at most kScanLoads samples and at least 2: 4 samples up to 4 elements a sample, 2 for |a - b| of 3 or 4 elements.
// Chosen from the register count the compiler reports for gfx950: with 4 samples everywhere (32 loads of |a - b| of 4 elements)
// the f64 walk kernel takes 94 VGPRs, 5 waves per SIMD; as below 62 (f32: 50), no scratch, 8 waves per SIMD.
SIXDOF_HOST_DEVICE constexpr uint32_t norms_depth(uint32_t count, bool minus) {
    const uint32_t per_sample = count * (minus ? 2u : 1u);
    const uint32_t d = kNormsMaxLoads / (per_sample ? per_sample : 1u);
    return d > kScanLoads ? kScanLoads : d < 2 ? 2 : d;
}

// The rule of this reader as norms_walk_as takes it (scan_walk's shape: sample + settled): every sample counts, so no walk ends early.
struct NormsRule {
    SIXDOF_HOST_DEVICE void sample(ExtremesRecord& rec, double s, uint64_t tick) const { norms_sample(rec, s, tick); }
    SIXDOF_HOST_DEVICE bool settled(const ExtremesRecord&) const { return false; }
};

// The record `r` after samples [lo, hi) of the range, in time order: sample j is the COUNT elements from a + slot(j) * stride_a
// (minus those from b + slot(j) * stride_b) at tick first_tick + j * every.  scan_walk's shape: the loads of norms_depth samples
// are issued before the first value is formed, the slot advances by an add and a compare, record and rule travel by value.
// rule.sample(r, s, tick) applies one squared norm; once rule.settled(r) says that no later sample can change what the reader
// reports, the walk stops loading (the norms never do; the norm events do: norm_events_plan.hpp).
template <class E, uint32_t COUNT, bool MINUS, class Record, class Rule>
SIXDOF_HOST_DEVICE inline Record norms_walk_as(Record r, const Rule rule, const E* __restrict__ a, const E* __restrict__ b, uint64_t stride_a, uint64_t stride_b,
                                               uint64_t lo, uint64_t hi, uint64_t first_tick, uint64_t every, uint64_t ring) {
    constexpr uint32_t kDepth = norms_depth(COUNT, MINUS);
    const uint64_t step = every % ring;
    uint64_t slot = sample_slot(first_tick, lo, every, ring), tick = first_tick + lo * every;
    uint64_t j = lo;
    for (; j + kDepth <= hi && !rule.settled(r); j += kDepth) {
        E xa[kDepth][COUNT], xb[kDepth][COUNT];
#pragma unroll
        for (uint32_t q = 0; q < kDepth; q++) {
            const E* __restrict__ pa = a + slot * stride_a;
            const E* __restrict__ pb = b + slot * stride_b;
#pragma unroll
            for (uint32_t e = 0; e < COUNT; e++) {
                xa[q][e] = pa[e];
                xb[q][e] = MINUS ? pb[e] : E(0);
            }
            slot = next_sample_slot(slot, step, ring);
        }
#pragma unroll
        for (uint32_t q = 0; q < kDepth; q++) {
            rule.sample(r, norms_value<E, COUNT, MINUS>(xa[q], xb[q]), tick);
            tick += every;
        }
    }
    for (; j < hi && !rule.settled(r); j++) {
        E xa[COUNT], xb[COUNT];
        const E* __restrict__ pa = a + slot * stride_a;
        const E* __restrict__ pb = b + slot * stride_b;
#pragma unroll
        for (uint32_t e = 0; e < COUNT; e++) {
            xa[e] = pa[e];
            xb[e] = MINUS ? pb[e] : E(0);
        }
        rule.sample(r, norms_value<E, COUNT, MINUS>(xa, xb), tick);
        slot = next_sample_slot(slot, step, ring);
        tick += every;
    }
    return r;
}
// The walk of probe `p` for run `run` of a world of n rows under `rule`.  A probe's shape is the same for every thread of a block
// (blockIdx.z names it), so the switch does not diverge.  norms_launch_ok has been asked.
template <class E, class Record, class Rule>
SIXDOF_HOST_DEVICE inline Record norms_walk_with(Record r, const Rule rule, const NormsProbe& p, uint64_t run, uint64_t n, uint32_t period, uint64_t lo, uint64_t hi,
                                                 uint64_t first_tick, uint64_t every, uint64_t ring) {
    const bool minus = (p.flags & kNormMinus) != 0;
    const E* a = static_cast<const E*>(p.ring_a) + (run * period + p.group_a) * p.w_a + p.element_a;
    const E* b = minus ? static_cast<const E*>(p.ring_b) + (run * period + p.group_b) * p.w_b + p.element_b : a;
    const uint64_t sa = n * p.w_a, sb = minus ? n * p.w_b : sa;
    switch (p.count * 2 + (minus ? 1u : 0u)) {
    case 2: return norms_walk_as<E, 1, false>(r, rule, a, b, sa, sb, lo, hi, first_tick, every, ring);
    case 3: return norms_walk_as<E, 1, true>(r, rule, a, b, sa, sb, lo, hi, first_tick, every, ring);
    case 4: return norms_walk_as<E, 2, false>(r, rule, a, b, sa, sb, lo, hi, first_tick, every, ring);
    case 5: return norms_walk_as<E, 2, true>(r, rule, a, b, sa, sb, lo, hi, first_tick, every, ring);
    case 6: return norms_walk_as<E, 3, false>(r, rule, a, b, sa, sb, lo, hi, first_tick, every, ring);
    case 7: return norms_walk_as<E, 3, true>(r, rule, a, b, sa, sb, lo, hi, first_tick, every, ring);
    case 8: return norms_walk_as<E, 4, false>(r, rule, a, b, sa, sb, lo, hi, first_tick, every, ring);
    case 9: return norms_walk_as<E, 4, true>(r, rule, a, b, sa, sb, lo, hi, first_tick, every, ring);
    default: return r;   // norms_launch_ok refuses such a probe
    }
}
// The norms' own walk: what norms_walk_kernel and the host twin both call.
template <class E>
SIXDOF_HOST_DEVICE inline ExtremesRecord norms_walk(ExtremesRecord r, const NormsProbe& p, uint64_t run, uint64_t n, uint32_t period, uint64_t lo, uint64_t hi,
                                                    uint64_t first_tick, uint64_t every, uint64_t ring) {
    return norms_walk_with<E>(r, NormsRule{}, p, run, n, period, lo, hi, first_tick, every, ring);
}

// Where the record of (segment, probe, run) sits in scratch: field f at base[f * runs], so that consecutive lanes store
// consecutive words; and where the six planes of (probe, run) sit in the output, `runs` doubles apart.
SIXDOF_HOST_DEVICE inline uint64_t norms_scratch_index(uint32_t seg, uint32_t n_probes, uint32_t probe, uint64_t runs, uint64_t run) {
    return (uint64_t(seg) * n_probes + probe) * kNormsFields * runs + run;
}
SIXDOF_HOST_DEVICE inline uint64_t norms_out_index(uint32_t probe, uint64_t runs, uint64_t run) { return uint64_t(probe) * kNormsPlanes * runs + run; }

// ---- geometry -------------------------------------------------------------------------------------------------------------
// Time segments of a read, scan_segments of (runs x probes, n_samples) under kNormsFillThreads, whose comment holds the measured
// table.  Unlike the events' walk no thread of this one stops early, and a sample is up to 8 loads; both walks are bound by the
// cache lines they touch (profiles/history_norms.md).
SIXDOF_HOST_DEVICE inline uint32_t norms_segments(uint64_t units, uint64_t n_samples) { return scan_segments(units, n_samples, kNormsFillThreads); }

// What launch_history_norms accepts, for the launcher (norms_kernels.hip) and its host twin (hip_fake.cpp) alike: 1 to 8 probes
// of 1 to 4 elements that lie within their component's rows, name rows of a run and carry known flags; whole runs, within the
// grid's x extent; 1 .. n_samples segments within the grid's y extent; ticks that a double holds.
inline bool norms_launch_ok(const NormsArgs& a, uint32_t n_probes, uint64_t n, uint32_t period, uint64_t first_tick, uint64_t n_samples, uint64_t every,
                            uint32_t segments) {
    if (n_probes == 0 || n_probes > kNormsMaxProbes || period == 0 || n % period != 0) return false;
    if (n_samples == 0 || (n_samples >> 32) || segments == 0 || segments > kScanMaxSegments || segments > n_samples) return false;
    if (!scan_ticks_ok(first_tick, n_samples, every)) return false;
    if ((n / period + kNormsThreads - 1) / kNormsThreads > 0x7fffffffull) return false;
    for (uint32_t k = 0; k < n_probes; k++) {
        const NormsProbe& p = a.p[k];
        if (p.count == 0 || p.count > kNormsMaxCount || (p.flags & ~kNormMinus)) return false;
        if (!p.ring_a || p.w_a == 0 || uint64_t(p.element_a) + p.count > p.w_a || p.group_a >= period) return false;
        if (n != 0 && n > ~uint64_t(0) / p.w_a) return false;
        if (p.flags & kNormMinus) {
            if (!p.ring_b || p.w_b == 0 || uint64_t(p.element_b) + p.count > p.w_b || p.group_b >= period) return false;
            if (n != 0 && n > ~uint64_t(0) / p.w_b) return false;
        }
    }
    return true;
}

}  // namespace sixdof
