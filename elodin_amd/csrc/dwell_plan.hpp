// dwell_plan.hpp — the record, the rule, the value and the geometry of the ring dwell: per condition and run, over the sampled
// ticks of a range, how long and how often a predicate held — finite samples, held samples, the maximal stretches of consecutive
// held samples and how many there are, the first and the last held tick, the stretch open at the start and the one open at the end,
// and the earliest stretch of maximal length.  The kernels (dwell_kernels.hip) and the host twin (hip_fake.cpp) run the same
// functions — dwell_walk, dwell_accumulate, dwell_merge —, sixdof_history_dwell (sixdof_capi.cpp) sizes its scratch with the
// geometry below, dwell_host_test.cpp checks all of it on the host.
//
// A run is `period` consecutive rows.  The value of a sample is formed in f64, every ring element widened first (exact for f32),
// without FMA contraction (SIXDOF_NO_CONTRACT on the device, -ffp-contract=off for the host twin): with kDwellElement the signed
// scalar v = a_0 or a_0 - b_0, one subtraction; with kDwellNormSq exactly the squared norm s of norms_plan.hpp's norms_value.  A
// sample is finite exactly when its value is; a non-finite one is skipped as the events skip it: it neither holds nor fails, and
// a stretch continues across it.  The predicate is an IEEE compare of the value against one or two finite levels.
//
// The rule is counts and ticks alone: pure integer, exact and associative in time order, so no result can depend on how the
// samples of a range are cut into segments, launches or calls.  Ticks are counts of completed ticks (never 0 for a sample, so 0
// means "none"), lengths are counted in finite samples.  The twelve output planes are the record itself, every word converted to
// the double that holds it (all are below 2^53 where scan_ticks_ok holds): dwell_emit and dwell_absorb are exact inverses, and
// the planes double as the accumulator a later call continues.
#pragma once

#include <cstddef>
#include <cstdint>

#include "events_plan.hpp"
#include "norms_plan.hpp"

namespace sixdof {

constexpr uint32_t kDwellThreads = 256;          // threads of a block, one run each
constexpr uint32_t kDwellPlanes = 12;            // SIXDOF_DWELL_PLANES: the record's words, in order
constexpr uint32_t kDwellFields = 12;            // 64-bit fields of a record in scratch
constexpr uint32_t kDwellMaxConditions = 8;      // SIXDOF_DWELL_MAX_CONDITIONS
constexpr uint32_t kDwellElement = 0, kDwellNormSq = 1;    // SIXDOF_DWELL_ELEMENT, SIXDOF_DWELL_NORM_SQ
constexpr uint32_t kDwellInside = 4, kDwellOutside = 5;    // SIXDOF_DWELL_INSIDE, SIXDOF_DWELL_OUTSIDE; 0 .. 3 are kEventLt .. kEventGe
// Threads below which the plan cuts the samples (dwell_segments).  Not derivable: it started from the norms' 16,384 — the walk is
// the norms', its lanes period * w elements apart —, and the forced-segment table of profiles/history_dwell.md (one |v| condition,
// 1,024 ticks, reduced only, one MI355X) confirms that value for this walk: at 1,024 runs 0.341 ms in one segment, 0.182 in 2,
// 0.102 in 4, 0.064 in 8, 0.049 in 16 and 0.050 in 32; at 65,536 runs 1.035 ms in one, 1.062 in 2, 1.084 in 4, 1.123 in 8 and 1.14
// from 16 on.  So the rule picks 16 at 1,024 runs (the table's minimum) and 1 at 65,536.  Sizes between the two, and the chain
// length, have not been measured.
constexpr uint64_t kDwellFillThreads = 16384;

struct DwellRecord {
    uint64_t count;                                      // finite samples
    uint64_t held;                                       // finite samples at which the predicate holds
    uint64_t entries;                                    // maximal stretches of consecutive held samples
    uint64_t first_held, last_held;                      // first / last tick at which it holds; 0: none
    uint64_t prefix_len, prefix_end;                     // the stretch that begins at the first finite sample, and its last tick
    uint64_t suffix_len, suffix_start;                   // the stretch that ends at the last finite sample, and its first tick
    uint64_t longest_len, longest_start, longest_end;    // the earliest stretch of maximal length
};
SIXDOF_HOST_DEVICE inline DwellRecord dwell_empty() { return {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; }

// One sample at tick t, later than every sample `rec` has met; `holds` is looked at only where `finite`.
SIXDOF_HOST_DEVICE inline void dwell_accumulate(DwellRecord& rec, uint64_t t, bool finite, bool holds) {
    // selects per field, not branches over groups of fields: the record stays in registers on the device
    const bool h = finite && holds, fails = finite && !holds;
    const bool opens = h && rec.suffix_len == 0;
    const bool leads = h && rec.prefix_len == rec.count;          // every finite sample so far has held
    rec.count += finite ? 1u : 0u;
    rec.held += h ? 1u : 0u;
    rec.entries += opens ? 1u : 0u;
    rec.first_held = h && rec.first_held == 0 ? t : rec.first_held;
    rec.last_held = h ? t : rec.last_held;
    rec.suffix_start = opens ? t : fails ? 0 : rec.suffix_start;
    rec.suffix_len = h ? rec.suffix_len + 1 : fails ? 0 : rec.suffix_len;
    rec.prefix_len += leads ? 1u : 0u;
    rec.prefix_end = leads ? t : rec.prefix_end;
    const bool longer = h && rec.suffix_len > rec.longest_len;   // strictly: of two stretches of one length the earlier stays
    rec.longest_len = longer ? rec.suffix_len : rec.longest_len;
    rec.longest_start = longer ? rec.suffix_start : rec.longest_start;
    rec.longest_end = longer ? t : rec.longest_end;
}
// `b` holds samples that all come after those of `a`.
SIXDOF_HOST_DEVICE inline DwellRecord dwell_merge(const DwellRecord& a, const DwellRecord& b) {
    if (a.count == 0) return b;
    if (b.count == 0) return a;
    DwellRecord r = a;
    const bool joined = a.suffix_len > 0 && b.prefix_len > 0;    // one stretch spans the cut
    r.count = a.count + b.count;
    r.held = a.held + b.held;
    r.entries = a.entries + b.entries - (joined ? 1u : 0u);
    r.first_held = a.first_held ? a.first_held : b.first_held;
    r.last_held = b.last_held ? b.last_held : a.last_held;
    if (a.prefix_len == a.count) {
        r.prefix_len = a.count + b.prefix_len;
        r.prefix_end = b.prefix_len ? b.prefix_end : a.prefix_end;
    }
    if (b.suffix_len == b.count) {
        r.suffix_len = a.suffix_len + b.count;
        r.suffix_start = a.suffix_len ? a.suffix_start : b.suffix_start;
    } else {
        r.suffix_len = b.suffix_len, r.suffix_start = b.suffix_start;
    }
    if (joined && a.suffix_len + b.prefix_len > r.longest_len)
        r.longest_len = a.suffix_len + b.prefix_len, r.longest_start = a.suffix_start, r.longest_end = b.prefix_end;
    if (b.longest_len > r.longest_len) r.longest_len = b.longest_len, r.longest_start = b.longest_start, r.longest_end = b.longest_end;
    return r;
}

// The predicate: v op lo for the one-sided ops, lo <= v <= hi and its complement for the two-sided ones.  v is finite.
SIXDOF_HOST_DEVICE inline bool dwell_holds(double v, uint32_t op, double lo, double hi) {
    return op == kDwellInside ? lo <= v && v <= hi : op == kDwellOutside ? v < lo || v > hi : events_holds(v, op, lo);
}
// One value, later than every sample `rec` has met.
SIXDOF_HOST_DEVICE inline void dwell_sample(DwellRecord& rec, double v, uint64_t tick, uint32_t op, double lo, double hi) {
    dwell_accumulate(rec, tick, QuantileBits<double>::finite(QuantileBits<double>::raw(v)), dwell_holds(v, op, lo, hi));
}
// The rule of one condition as norms_walk_as takes it: every sample counts, so no walk ends early.
struct DwellRule {
    double lo, hi;
    uint32_t op;
    SIXDOF_HOST_DEVICE void sample(DwellRecord& rec, double v, uint64_t tick) const { dwell_sample(rec, v, tick, op, lo, hi); }
    SIXDOF_HOST_DEVICE bool settled(const DwellRecord&) const { return false; }
};

// The twelve planes of one (condition, run), `plane_stride` doubles apart, and the record they came from: conversions only, an
// integer below 2^53 to the double that holds it and back.
SIXDOF_HOST_DEVICE inline void dwell_emit(const DwellRecord& r, double* out, uint64_t plane_stride) {
    out[0] = static_cast<double>(r.count), out[plane_stride] = static_cast<double>(r.held), out[2 * plane_stride] = static_cast<double>(r.entries);
    out[3 * plane_stride] = static_cast<double>(r.first_held), out[4 * plane_stride] = static_cast<double>(r.last_held);
    out[5 * plane_stride] = static_cast<double>(r.prefix_len), out[6 * plane_stride] = static_cast<double>(r.prefix_end);
    out[7 * plane_stride] = static_cast<double>(r.suffix_len), out[8 * plane_stride] = static_cast<double>(r.suffix_start);
    out[9 * plane_stride] = static_cast<double>(r.longest_len), out[10 * plane_stride] = static_cast<double>(r.longest_start);
    out[11 * plane_stride] = static_cast<double>(r.longest_end);
}
SIXDOF_HOST_DEVICE inline DwellRecord dwell_absorb(const double* out, uint64_t plane_stride) {
    return {static_cast<uint64_t>(out[0]),
            static_cast<uint64_t>(out[plane_stride]),
            static_cast<uint64_t>(out[2 * plane_stride]),
            static_cast<uint64_t>(out[3 * plane_stride]),
            static_cast<uint64_t>(out[4 * plane_stride]),
            static_cast<uint64_t>(out[5 * plane_stride]),
            static_cast<uint64_t>(out[6 * plane_stride]),
            static_cast<uint64_t>(out[7 * plane_stride]),
            static_cast<uint64_t>(out[8 * plane_stride]),
            static_cast<uint64_t>(out[9 * plane_stride]),
            static_cast<uint64_t>(out[10 * plane_stride]),
            static_cast<uint64_t>(out[11 * plane_stride])};
}
// A record in scratch: field f of unit u at base[f * stride + u], so that consecutive lanes store consecutive words.
SIXDOF_HOST_DEVICE inline void dwell_store(const DwellRecord& r, uint64_t* base, uint64_t stride) {
    base[0] = r.count, base[stride] = r.held, base[2 * stride] = r.entries, base[3 * stride] = r.first_held, base[4 * stride] = r.last_held;
    base[5 * stride] = r.prefix_len, base[6 * stride] = r.prefix_end, base[7 * stride] = r.suffix_len, base[8 * stride] = r.suffix_start;
    base[9 * stride] = r.longest_len, base[10 * stride] = r.longest_start, base[11 * stride] = r.longest_end;
}
SIXDOF_HOST_DEVICE inline DwellRecord dwell_load(const uint64_t* base, uint64_t stride) {
    return {base[0],          base[stride],     base[2 * stride], base[3 * stride], base[4 * stride],  base[5 * stride],
            base[6 * stride], base[7 * stride], base[8 * stride], base[9 * stride], base[10 * stride], base[11 * stride]};
}

// One condition as the kernels see it: the probe of norms_plan.hpp, what is formed of it and the predicate.
struct DwellCondition {
    NormsProbe probe;
    double lo, hi;        // finite; hi is 0 with a one-sided op, lo <= hi with a two-sided one; not below 0 with kDwellNormSq
    uint32_t kind, op;    // kDwellElement, kDwellNormSq; kEventLt .. kEventGe, kDwellInside, kDwellOutside
};
struct DwellArgs { DwellCondition c[kDwellMaxConditions]; };   // by value: 576 bytes of kernel arguments
static_assert(sizeof(DwellCondition) == 72 && sizeof(DwellArgs) == 576, "DwellArgs is 8 x 72 bytes");

// ---- the value and the walk -----------------------------------------------------------------------------------------------
// The signed scalar of one sample of a kDwellElement condition.  `xb` is not read without MINUS.
template <class E, bool MINUS>
SIXDOF_HOST_DEVICE inline double dwell_element_value(E xa, E xb) {
    SIXDOF_NO_CONTRACT
    double d = static_cast<double>(xa);
    if (MINUS) d = d - static_cast<double>(xb);
    return d;
}
// norms_walk_as for one element whose value is d_0, not d_0 * d_0: the same slots, ticks and norms_depth(1, MINUS) loads in
// flight before the first value is formed.
template <class E, bool MINUS>
SIXDOF_HOST_DEVICE inline DwellRecord dwell_element_walk_as(DwellRecord r, const DwellRule rule, const E* __restrict__ a, const E* __restrict__ b, uint64_t stride_a,
                                                            uint64_t stride_b, uint64_t lo, uint64_t hi, uint64_t first_tick, uint64_t every, uint64_t ring) {
    constexpr uint32_t kDepth = norms_depth(1, MINUS);
    const uint64_t step = every % ring;
    uint64_t slot = sample_slot(first_tick, lo, every, ring), tick = first_tick + lo * every;
    uint64_t j = lo;
    for (; j + kDepth <= hi; j += kDepth) {
        E xa[kDepth], xb[kDepth];
#pragma unroll
        for (uint32_t q = 0; q < kDepth; q++) {
            xa[q] = a[slot * stride_a];
            xb[q] = MINUS ? b[slot * stride_b] : E(0);
            slot = next_sample_slot(slot, step, ring);
        }
#pragma unroll
        for (uint32_t q = 0; q < kDepth; q++) {
            rule.sample(r, dwell_element_value<E, MINUS>(xa[q], xb[q]), tick);
            tick += every;
        }
    }
    for (; j < hi; j++) {
        const E xa = a[slot * stride_a], xb = MINUS ? b[slot * stride_b] : E(0);
        rule.sample(r, dwell_element_value<E, MINUS>(xa, xb), tick);
        slot = next_sample_slot(slot, step, ring);
        tick += every;
    }
    return r;
}
// The record `r` after samples [lo, hi) of condition `c` for run `run` of a world of n rows: what dwell_walk_kernel and the host
// twin both call.  A condition's shape is the same for every thread of a block (blockIdx.z names it), so no branch diverges.
// dwell_launch_ok has been asked.
template <class E>
SIXDOF_HOST_DEVICE inline DwellRecord dwell_walk(DwellRecord r, const DwellCondition& c, uint64_t run, uint64_t n, uint32_t period, uint64_t lo, uint64_t hi,
                                                 uint64_t first_tick, uint64_t every, uint64_t ring) {
    const DwellRule rule{c.lo, c.hi, c.op};
    if (c.kind == kDwellNormSq) return norms_walk_with<E>(r, rule, c.probe, run, n, period, lo, hi, first_tick, every, ring);
    const NormsProbe& p = c.probe;
    const bool minus = (p.flags & kNormMinus) != 0;
    const E* a = static_cast<const E*>(p.ring_a) + (run * period + p.group_a) * p.w_a + p.element_a;
    const E* b = minus ? static_cast<const E*>(p.ring_b) + (run * period + p.group_b) * p.w_b + p.element_b : a;
    const uint64_t sa = n * p.w_a, sb = minus ? n * p.w_b : sa;
    return minus ? dwell_element_walk_as<E, true>(r, rule, a, b, sa, sb, lo, hi, first_tick, every, ring)
                 : dwell_element_walk_as<E, false>(r, rule, a, b, sa, sb, lo, hi, first_tick, every, ring);
}

// Where the record of (segment, condition, run) sits in scratch: field f at base[f * runs], so that consecutive lanes store
// consecutive words; and where the twelve planes of (condition, run) sit in the output, `runs` doubles apart.
SIXDOF_HOST_DEVICE inline uint64_t dwell_scratch_index(uint32_t seg, uint32_t n_conditions, uint32_t cond, uint64_t runs, uint64_t run) {
    return (uint64_t(seg) * n_conditions + cond) * kDwellFields * runs + run;
}
SIXDOF_HOST_DEVICE inline uint64_t dwell_out_index(uint32_t cond, uint64_t runs, uint64_t run) { return uint64_t(cond) * kDwellPlanes * runs + run; }

// ---- geometry -------------------------------------------------------------------------------------------------------------
// Time segments of a read, scan_segments of (runs x conditions, n_samples) under kDwellFillThreads.
SIXDOF_HOST_DEVICE inline uint32_t dwell_segments(uint64_t units, uint64_t n_samples) { return scan_segments(units, n_samples, kDwellFillThreads); }

// What the header asks of one condition's kind, op and levels, for dwell_launch_ok and sixdof_history_dwell alike; 0: nothing,
// otherwise what is wrong, in words.
inline const char* dwell_condition_fault(uint32_t kind, uint32_t op, uint32_t count, double lo, double hi) {
    const auto finite = [](double x) { return QuantileBits<double>::finite(QuantileBits<double>::raw(x)); };
    if (kind > kDwellNormSq) return "unknown kind";
    if (op > kDwellOutside) return "unknown op";
    if (kind == kDwellElement && count != 1) return "SIXDOF_DWELL_ELEMENT reads one element: count must be 1";
    if (!finite(lo) || !finite(hi)) return "a level is not finite";
    if (op <= kEventGe && hi != 0.0) return "hi must be 0 with a one-sided op";
    if (op > kEventGe && lo > hi) return "lo is above hi";
    if (kind == kDwellNormSq && (lo < 0.0 || hi < 0.0)) return "a squared level is below 0";
    return nullptr;
}
// What launch_history_dwell accepts, for the launcher (dwell_kernels.hip) and its host twin (hip_fake.cpp) alike: what
// norms_launch_ok asks of the probes and the range, and conditions without a dwell_condition_fault.
inline bool dwell_launch_ok(const DwellArgs& a, uint32_t n_conditions, uint64_t n, uint32_t period, uint64_t first_tick, uint64_t n_samples, uint64_t every,
                            uint32_t segments) {
    if (n_conditions == 0 || n_conditions > kDwellMaxConditions) return false;
    NormsArgs probes{};
    for (uint32_t k = 0; k < n_conditions; k++) {
        const DwellCondition& c = a.c[k];
        if (dwell_condition_fault(c.kind, c.op, c.probe.count, c.lo, c.hi)) return false;
        probes.p[k] = c.probe;
    }
    static_assert(kDwellMaxConditions == kNormsMaxProbes && kDwellThreads == kNormsThreads, "the probes are checked by norms_launch_ok");
    return norms_launch_ok(probes, n_conditions, n, period, first_tick, n_samples, every, segments);
}

}  // namespace sixdof
