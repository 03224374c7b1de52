// dwell_host_test.cpp — sixdof_history_dwell (sixdof_capi.cpp) over the fake runtime (hip_fake.cpp), whose launcher walks and merges
// through dwell_plan.hpp — dwell_walk, dwell_accumulate and dwell_merge, the functions the kernels call — in the kernels' time
// segments, under AddressSanitizer / UBSan and without FMA contraction, no GPU: `make dwell_test`, tests/test_history_dwell_host.py.
//
// The ring and the fault sweep are ring_host_fixture.hpp's.  Checked: the rule against a plain loop written here — every sequence
// over {holds, fails, skipped} up to length 8 and random ones up to 200, every cut into 2 and 3 parts merged in both association
// orders, accumulate against the merge of a one-sample record, crafted ties; value and predicate bitwise against a plain loop,
// both kinds, all six ops, f32 and f64, with and without MINUS, over +-0 at a level of 0, denormals, an overflowing difference and
// an overflowing square, NaN, +-inf and values that equal a level; all twelve planes against a plain loop over the fixture's host
// copy of the ring, the ring wrapped; one call against the same range in 2 and 3 calls (SIXDOF_DWELL_HOLD, then
// SIXDOF_DWELL_CONTINUE) and under forced segment counts, one sample per segment included; every refusal with nothing copied and
// the accumulator untouched; the conditions of SIXDOF_DWELL_CONTINUE; every fallible runtime call failed once.
#include <algorithm>

#include "dwell_plan.hpp"
#include "ring_host_fixture.hpp"

namespace {

constexpr size_t kPlanes = SIXDOF_DWELL_PLANES;
constexpr uint32_t kHold = SIXDOF_DWELL_HOLD, kContinue = SIXDOF_DWELL_CONTINUE, kMinus = SIXDOF_NORM_MINUS;
constexpr uint32_t kElement = SIXDOF_DWELL_ELEMENT, kNormSq = SIXDOF_DWELL_NORM_SQ;
constexpr uint32_t kLt = SIXDOF_EVENT_LT, kLe = SIXDOF_EVENT_LE, kGt = SIXDOF_EVENT_GT, kGe = SIXDOF_EVENT_GE, kInside = SIXDOF_DWELL_INSIDE, kOutside = SIXDOF_DWELL_OUTSIDE;
static_assert(sizeof(sixdof_dwell_condition) == 64 && offsetof(sixdof_dwell_condition, lo) == 40 && offsetof(sixdof_dwell_condition, hi) == 48 &&
                  offsetof(sixdof_dwell_condition, kind) == 56 && offsetof(sixdof_dwell_condition, op) == 60,
              "sixdof_dwell_condition is 64 bytes");
static_assert(kPlanes == sixdof::kDwellPlanes && SIXDOF_DWELL_MAX_CONDITIONS == sixdof::kDwellMaxConditions && kInside == sixdof::kDwellInside &&
                  kOutside == sixdof::kDwellOutside && kElement == sixdof::kDwellElement && kNormSq == sixdof::kDwellNormSq,
              "the header's constants are the plan's");

void force_segments(uint64_t count) { force_segments("SIXDOF_DWELL_SEGMENTS", count); }
const double kNaN = std::numeric_limits<double>::quiet_NaN();
const double kInf = std::numeric_limits<double>::infinity();

uint64_t bits_of(double x) { uint64_t u; std::memcpy(&u, &x, 8); return u; }

// ---- the plain statements: the issue's words, one sample after the other, nothing kept between samples but the list ----------
// One sample: 0 fails, 1 holds, 2 skipped (not finite).
struct PlainSample { int state; uint64_t tick; };
// The twelve words of a sequence, from the list of its finite samples and the stretches found in it.
std::vector<uint64_t> plain_words(const std::vector<PlainSample>& all) {
    std::vector<PlainSample> f;
    for (const PlainSample& s : all)
        if (s.state != 2) f.push_back(s);
    struct Stretch { size_t first, last; };
    std::vector<Stretch> stretches;
    uint64_t held = 0;
    for (size_t i = 0; i < f.size(); i++) {
        if (!f[i].state) continue;
        held++;
        if (i > 0 && f[i - 1].state) stretches.back().last = i;
        else stretches.push_back({i, i});
    }
    std::vector<uint64_t> w(kPlanes, 0);
    w[0] = f.size(), w[1] = held, w[2] = stretches.size();
    if (stretches.empty()) return w;
    w[3] = f[stretches.front().first].tick, w[4] = f[stretches.back().last].tick;
    if (stretches.front().first == 0) w[5] = stretches.front().last + 1, w[6] = f[stretches.front().last].tick;
    if (stretches.back().last + 1 == f.size()) w[7] = stretches.back().last - stretches.back().first + 1, w[8] = f[stretches.back().first].tick;
    for (const Stretch& s : stretches)
        if (s.last - s.first + 1 > w[9]) w[9] = s.last - s.first + 1, w[10] = f[s.first].tick, w[11] = f[s.last].tick;
    return w;
}
std::vector<uint64_t> words_of(const sixdof::DwellRecord& r) {
    return {r.count, r.held, r.entries, r.first_held, r.last_held, r.prefix_len, r.prefix_end, r.suffix_len, r.suffix_start, r.longest_len, r.longest_start, r.longest_end};
}
template <class T>
double plain_element(const T* a, const T* b, bool minus) {
    const double a0 = a[0];
    if (!minus) return a0;
    const double b0 = b[0];
    return a0 - b0;
}
template <class T>
double plain_norm_sq(const T* a, const T* b, uint32_t count, bool minus) {
    double s = 0.0;
    for (uint32_t e = 0; e < count; e++) {
        const double ae = a[e];
        double d = ae;
        if (minus) {
            const double be = b[e];
            d = ae - be;
        }
        const double square = d * d;
        if (e == 0) s = square;
        else s = s + square;
    }
    return s;
}
int plain_state(double v, uint32_t op, double lo, double hi) {
    if (!std::isfinite(v)) return 2;
    switch (op) {
    case kLt: return v < lo;
    case kLe: return v <= lo;
    case kGt: return v > lo;
    case kGe: return v >= lo;
    case kInside: return lo <= v && v <= hi;
    default: return v < lo || v > hi;
    }
}

// ---- the rule -------------------------------------------------------------------------------------------------------------
uint64_t g_merges = 0;
// One sequence of states: the walk, every cut in 2, every cut in 3 in both association orders, against the plain loop.
void rule_of_sequence(const std::vector<int>& states, bool every_cut_in_3, std::mt19937_64& rng) {
    using namespace sixdof;
    const uint32_t len = static_cast<uint32_t>(states.size());
    std::vector<PlainSample> all;
    for (uint32_t j = 0; j < len; j++) all.push_back({states[j], 10 + 3 * uint64_t(j)});
    auto walk = [&](uint32_t lo, uint32_t hi) {
        DwellRecord r = dwell_empty();
        for (uint32_t j = lo; j < hi; j++) dwell_accumulate(r, all[j].tick, all[j].state != 2, all[j].state == 1);
        return r;
    };
    const std::vector<uint64_t> want = plain_words(all);
    if (words_of(walk(0, len)) != want) return complain("rule: a sequence of length " + std::to_string(len) + " differs from the plain loop");
    auto check = [&](const DwellRecord& merged, const char* what) {
        if (words_of(merged) != want) complain(std::string("rule: ") + what + " of a sequence of length " + std::to_string(len) + " differs from one walk");
        g_merges++;
    };
    // accumulate is the merge of a one-sample record
    DwellRecord by_merge = dwell_empty();
    for (uint32_t j = 0; j < len; j++) by_merge = dwell_merge(by_merge, walk(j, j + 1));
    check(by_merge, "the merge of one-sample records");
    auto three = [&](uint32_t c1, uint32_t c2) {
        check(dwell_merge(dwell_merge(walk(0, c1), walk(c1, c2)), walk(c2, len)), "a cut in 3, left first");
        check(dwell_merge(walk(0, c1), dwell_merge(walk(c1, c2), walk(c2, len))), "a cut in 3, right first");
    };
    for (uint32_t c1 = 0; c1 <= len; c1++) {
        check(dwell_merge(walk(0, c1), walk(c1, len)), "a cut in 2");
        for (uint32_t c2 = c1; every_cut_in_3 && c2 <= len; c2++) three(c1, c2);
    }
    for (int k = 0; !every_cut_in_3 && k < 400; k++) {
        const uint32_t x = static_cast<uint32_t>(rng() % (len + 1)), y = static_cast<uint32_t>(rng() % (len + 1));
        three(std::min(x, y), std::max(x, y));
    }
}
void rule_over_cuts() {
    using namespace sixdof;
    std::mt19937_64 rng(11);
    uint64_t sequences = 0, pairs = 0;
    for (uint32_t len = 0; len <= 8; len++) {
        uint64_t total = 1;
        for (uint32_t k = 0; k < len; k++) total *= 3;
        for (uint64_t code = 0; code < total; code++) {
            std::vector<int> states(len);
            uint64_t c = code;
            for (uint32_t k = 0; k < len; k++) states[k] = int(c % 3), c /= 3;
            rule_of_sequence(states, true, rng);
            sequences++, pairs += uint64_t(len + 1) * (len + 2) / 2;
        }
    }
    std::printf("dwell_host_test: %llu sequences up to length 8, %llu cut pairs exhaustively\n", static_cast<unsigned long long>(sequences), static_cast<unsigned long long>(pairs));
    for (int k = 0; k < 120; k++) {
        std::vector<int> states(1 + rng() % 200);
        const uint64_t hold_share = 1 + rng() % 9;       // long stretches in some, short ones in others
        for (int& s : states) s = rng() % 10 == 0 ? 2 : rng() % 10 < hold_share ? 1 : 0;
        rule_of_sequence(states, false, rng);
    }
    // crafted ties: of two stretches of one length the EARLIER is the longest, however the sequence is cut
    {
        const std::vector<int> tie = {1, 1, 0, 1, 1, 0, 2, 1, 2, 1, 0};    // ticks 10 13 | 19 22 | 31 (34) 37: three stretches of 2
        rule_of_sequence(tie, true, rng);
        DwellRecord r = dwell_empty();
        for (size_t j = 0; j < tie.size(); j++) dwell_accumulate(r, 10 + 3 * j, tie[j] != 2, tie[j] == 1);
        if (r.longest_len != 2 || r.longest_start != 10 || r.longest_end != 13 || r.entries != 3 || r.held != 6 || r.count != 9) complain("rule: a tie does not report the earlier stretch");
        // the joined stretch ties with a's longest: a's stays; b's longest ties with the joined one: the joined one stays
        DwellRecord a = dwell_empty(), b = dwell_empty();
        for (int s : {1, 1, 0, 1}) dwell_accumulate(a, 1 + a.count, true, s == 1);      // ticks 1 2 (3) 4
        for (int s : {1, 0, 1, 1}) dwell_accumulate(b, 5 + b.count, true, s == 1);      // ticks 5 (6) 7 8
        const DwellRecord m = dwell_merge(a, b);
        if (m.longest_len != 2 || m.longest_start != 1 || m.longest_end != 2 || m.entries != 3) complain("rule: a joined stretch that ties replaces the earlier one");
        DwellRecord c = dwell_empty();
        for (int s : {0, 1}) dwell_accumulate(c, 1 + c.count, true, s == 1);            // ticks (1) 2
        const DwellRecord m2 = dwell_merge(c, b);                                       // 2 5 joined: length 2, ties with 7 8
        if (m2.longest_len != 2 || m2.longest_start != 2 || m2.longest_end != 5 || m2.entries != 2) complain("rule: b's stretch that ties replaces the joined one");
        // a stretch continues across a skipped sample, and a skipped sample alone leaves the record empty
        DwellRecord s = dwell_empty();
        dwell_accumulate(s, 7, false, true);
        if (words_of(s) != words_of(dwell_empty())) complain("rule: a skipped sample changes the record");
    }
    // emit and absorb are exact inverses, near 2^53 too
    {
        const uint64_t top = (uint64_t(1) << 53) - 1;
        const DwellRecord r{top, top - 1, top - 2, top - 3, top - 4, top - 5, top - 6, top - 7, top - 8, top - 9, top - 10, top - 11};
        double planes[kPlanes * 3];
        uint64_t stored[kPlanes * 3];
        dwell_emit(r, planes + 1, 3), dwell_store(r, stored + 2, 3);
        if (words_of(dwell_absorb(planes + 1, 3)) != words_of(r) || words_of(dwell_load(stored + 2, 3)) != words_of(r)) complain("rule: absorb / load is not the inverse of emit / store");
        for (uint32_t f = 0; f < kPlanes; f++)
            if (planes[1 + 3 * f] != double(top - f) || stored[2 + 3 * f] != top - f) complain("rule: plane " + std::to_string(f) + " is not the record's word " + std::to_string(f));
    }
    std::printf("dwell_host_test: %llu merges of every cut in 2 and 3 agree with one walk\n", static_cast<unsigned long long>(g_merges));
}

// ---- the value and the predicate ------------------------------------------------------------------------------------------
// The state the plan gives one value under one condition: through DwellRule, as the walks do.
int compiled_state(double v, uint32_t op, double lo, double hi) {
    sixdof::DwellRecord r = sixdof::dwell_empty();
    sixdof::DwellRule{lo, hi, op}.sample(r, v, 5);
    return r.count == 0 ? 2 : int(r.held);
}
template <class T>
void value_function() {
    using L = std::numeric_limits<T>;
    const T big = T(std::sqrt(double(L::max())));
    const std::vector<T> pool = {T(0.0), T(-0.0), L::denorm_min(), -L::denorm_min(), L::min(), T(1), T(-1), T(3), T(-4), T(0.1), T(1e-30), big, -big, L::max(), L::lowest(),
                                 L::quiet_NaN(), L::infinity(), -L::infinity(), T(6.4e6), T(6.4e6 + 1)};
    const uint32_t ops[6] = {kLt, kLe, kGt, kGe, kInside, kOutside};
    std::mt19937_64 rng(sizeof(T));
    uint64_t checked = 0, overflowed = 0, equal_level = 0, skipped = 0;
    // the element: every pair of the pool, with and without MINUS; levels: 0 (+-0 compare equal), the value itself (v == lo, v == hi), others
    for (size_t i = 0; i < pool.size(); i++)
        for (size_t j = 0; j < pool.size(); j++)
            for (int minus = 0; minus < 2; minus++) {
                const T a[1] = {pool[i]}, b[1] = {pool[j]};
                const double want = plain_element(a, b, minus != 0);
                const double got = minus ? sixdof::dwell_element_value<T, true>(a[0], b[0]) : sixdof::dwell_element_value<T, false>(a[0], b[0]);
                if (std::isfinite(want) != std::isfinite(got) || (std::isfinite(want) && bits_of(want) != bits_of(got))) return complain("value: an element differs from the plain loop");
                overflowed += std::isfinite(double(a[0])) && std::isfinite(double(b[0])) && !std::isfinite(got);
                const double v = std::isfinite(want) ? want : 0.0;
                const double levels[][2] = {{0.0, 0.0}, {-0.0, 0.0}, {v, v}, {v, std::fabs(v) + 1.0}, {-std::fabs(v) - 1.0, v}, {-1.0, 1.0}, {1e-300, 1e300}, {-1e300, -1e-300}};
                for (const auto& lv : levels)
                    for (uint32_t op : ops) {
                        const double lo = lv[0], hi = op <= kGe ? 0.0 : lv[1];
                        const int state = plain_state(want, op, lo, hi);
                        if (compiled_state(got, op, lo, hi) != state) return complain("predicate: an element under op " + std::to_string(op) + " differs from the plain loop");
                        equal_level += state != 2 && (want == lo || want == hi);
                        skipped += state == 2;
                        checked++;
                    }
            }
    if (sizeof(T) == 8 && overflowed == 0) complain("value: no difference overflowed from finite inputs");
    if (sizeof(T) == 4) {      // f32 is widened first: the largest float minus the lowest is a finite double
        if (!std::isfinite(sixdof::dwell_element_value<T, true>(L::max(), L::lowest()))) complain("value: f32 was not widened before the subtraction");
    } else if (std::isfinite(sixdof::dwell_element_value<T, true>(L::max(), L::lowest()))) {
        complain("value: an overflowing difference is finite");
    }
    // -0.0 at a level of 0: equal, so >= and <= hold, > and < do not, inside [0, 0] holds
    if (compiled_state(-0.0, kGe, 0.0, 0.0) != 1 || compiled_state(-0.0, kLt, 0.0, 0.0) != 0 || compiled_state(0.0, kLe, -0.0, 0.0) != 1 || compiled_state(-0.0, kInside, 0.0, 0.0) != 1 ||
        compiled_state(-0.0, kOutside, 0.0, 0.0) != 0)
        complain("predicate: -0.0 is not equal to a level of 0");
    // the squared norm: exactly norms_value, the value the walk hands the rule; squared levels
    uint64_t sq_overflowed = 0;
    for (uint32_t count = 1; count <= 4; count++)
        for (int minus = 0; minus < 2; minus++)
            for (size_t i = 0; i < pool.size(); i++)
                for (size_t j = 0; j < pool.size(); j++) {
                    T a[4], b[4];
                    a[0] = pool[i], b[0] = pool[j];
                    for (uint32_t e = 1; e < 4; e++) a[e] = (i + j + e) % 3 ? T(double(rng() % 977) / 7.0) : pool[rng() % pool.size()], b[e] = T(double(rng() % 1000003) * 1e-3);
                    const double want = plain_norm_sq(a, b, count, minus != 0);
                    double got = 0;
                    switch (count * 2 + minus) {
                    case 2: got = sixdof::norms_value<T, 1, false>(a, b); break;
                    case 3: got = sixdof::norms_value<T, 1, true>(a, b); break;
                    case 4: got = sixdof::norms_value<T, 2, false>(a, b); break;
                    case 5: got = sixdof::norms_value<T, 2, true>(a, b); break;
                    case 6: got = sixdof::norms_value<T, 3, false>(a, b); break;
                    case 7: got = sixdof::norms_value<T, 3, true>(a, b); break;
                    case 8: got = sixdof::norms_value<T, 4, false>(a, b); break;
                    default: got = sixdof::norms_value<T, 4, true>(a, b); break;
                    }
                    if (std::isfinite(want) != std::isfinite(got) || (std::isfinite(want) && bits_of(want) != bits_of(got))) return complain("value: a squared norm differs from the plain loop");
                    bool inputs_finite = true;
                    for (uint32_t e = 0; e < count; e++) inputs_finite = inputs_finite && std::isfinite(double(a[e])) && (!minus || std::isfinite(double(b[e])));
                    sq_overflowed += inputs_finite && !std::isfinite(got);
                    const double v = std::isfinite(want) ? want : 1.0;
                    const double levels[][2] = {{0.0, 0.0}, {v, v}, {v, v + 1.0}, {0.0, v}, {1.0, 1e300}};
                    for (const auto& lv : levels)
                        for (uint32_t op : ops) {
                            const double lo = lv[0], hi = op <= kGe ? 0.0 : lv[1];
                            const int state = plain_state(want, op, lo, hi);
                            if (compiled_state(got, op, lo, hi) != state) return complain("predicate: a squared norm under op " + std::to_string(op) + " differs from the plain loop");
                            equal_level += state != 2 && (want == lo || want == hi);
                            skipped += state == 2;
                            checked++;
                        }
                }
    if (sizeof(T) == 8 && sq_overflowed == 0) complain("value: no square overflowed from finite inputs");
    if (equal_level == 0 || skipped == 0) complain("value: no value met a level, or none was skipped");
    std::printf("dwell_host_test: %llu %s values and predicates agree with the plain loop\n", static_cast<unsigned long long>(checked), sizeof(T) == 4 ? "f32" : "f64");
}

void plan_arithmetic() {
    using namespace sixdof;
    if (dwell_segments(65536, 1024) != 1 || dwell_segments(kDwellFillThreads, 1024) != 1 || dwell_segments(1024, 8) != 1 || dwell_segments(0, 100) != 1 ||
        dwell_segments(1024, 1024) != (kDwellFillThreads + 1023) / 1024)
        complain("plan: dwell_segments");
    if (dwell_scratch_index(2, 3, 1, 10, 4) != (2 * 3 + 1) * 12 * 10 + 4 || dwell_out_index(2, 10, 4) != 2 * 12 * 10 + 4) complain("plan: indices");
    if (dwell_condition_fault(kElement, kGt, 1, 0.5, 0.0) || dwell_condition_fault(kNormSq, kInside, 4, 0.0, 2.0) || dwell_condition_fault(kElement, kOutside, 1, -1.0, -1.0) ||
        dwell_condition_fault(kNormSq, kLe, 3, 0.0, -0.0))
        complain("plan: a good condition has a fault");
    if (!dwell_condition_fault(2, kGt, 1, 0, 0) || !dwell_condition_fault(kElement, 6, 1, 0, 0) || !dwell_condition_fault(kElement, kGt, 2, 0, 0) ||
        !dwell_condition_fault(kElement, kGt, 1, kNaN, 0) || !dwell_condition_fault(kElement, kInside, 1, 0, kInf) || !dwell_condition_fault(kElement, kGe, 1, 0, 1) ||
        !dwell_condition_fault(kElement, kInside, 1, 2, 1) || !dwell_condition_fault(kElement, kOutside, 1, 2, 1) || !dwell_condition_fault(kNormSq, kGt, 1, -1, 0) ||
        !dwell_condition_fault(kNormSq, kInside, 1, -1, 1))
        complain("plan: a bad condition has no fault");
    DwellArgs a{};
    int dummy = 0;
    a.c[0] = {{&dummy, &dummy, 7, 6, 4, 3, 3, 0, 1, kNormMinus}, -1.0, 1.0, kDwellElement, kDwellInside};
    auto ok = [&] { return dwell_launch_ok(a, 1, 8, 4, 1, 10, 1, 2); };
    if (!ok()) complain("plan: dwell_launch_ok refuses a good launch");
    const DwellArgs good = a;
    a.c[0].probe.count = 2; if (ok()) complain("plan: count 2 of an element"); a = good;
    a.c[0].kind = kDwellNormSq; if (ok()) complain("plan: a negative squared level"); a = good;
    a.c[0].kind = 2; if (ok()) complain("plan: kind"); a = good;
    a.c[0].op = 6; if (ok()) complain("plan: op"); a = good;
    a.c[0].lo = 2.0; if (ok()) complain("plan: lo above hi"); a = good;
    a.c[0].op = kEventGt; if (ok()) complain("plan: hi with a one-sided op"); a = good;
    a.c[0].probe.element_a = 7; if (ok()) complain("plan: element"); a = good;
    a.c[0].probe.group_b = 4; if (ok()) complain("plan: minus group"); a = good;
    if (dwell_launch_ok(a, 0, 8, 4, 1, 10, 1, 2) || dwell_launch_ok(a, 9, 8, 4, 1, 10, 1, 2) || dwell_launch_ok(a, 1, 9, 4, 1, 10, 1, 2) || dwell_launch_ok(a, 1, 8, 0, 1, 10, 1, 2) ||
        dwell_launch_ok(a, 1, 8, 4, 1, 10, 1, 11) || dwell_launch_ok(a, 1, 8, 4, 1, 10, 1, 0) || dwell_launch_ok(a, 1, 8, 4, uint64_t(1) << 53, 1, 1, 1))
        complain("plan: dwell_launch_ok accepts a bad launch");
}

// ---- reads over the fixture's ring ----------------------------------------------------------------------------------------
int column_of(uint64_t id) {
    for (int k = 0; k < 4; k++)
        if (id == sixdof_component_id(kNames[k])) return k;
    return -1;
}
sixdof_dwell_condition condition(uint32_t kind, uint32_t op, double lo, double hi, const char* name, uint32_t element, uint32_t count, uint32_t group = 0) {
    sixdof_dwell_condition c{};
    c.probe.component_id = sixdof_component_id(name), c.probe.element = element, c.probe.count = count, c.probe.group = group;
    c.lo = lo, c.hi = hi, c.kind = kind, c.op = op;
    return c;
}
sixdof_dwell_condition condition(uint32_t kind, uint32_t op, double lo, double hi, const char* name, uint32_t element, uint32_t count, uint32_t group, const char* minus,
                                 uint32_t minus_element, uint32_t minus_group) {
    sixdof_dwell_condition c = condition(kind, op, lo, hi, name, element, count, group);
    c.probe.flags = kMinus, c.probe.minus_component_id = sixdof_component_id(minus), c.probe.minus_element = minus_element, c.probe.minus_group = minus_group;
    return c;
}

template <class T>
std::vector<double> plain_loop(const Recorded<T>& r, const std::vector<sixdof_dwell_condition>& conditions, uint32_t period, const std::vector<uint64_t>& ticks) {
    const uint64_t runs = r.n / period;
    std::vector<double> out(conditions.size() * kPlanes * runs, kNaN);
    for (size_t k = 0; k < conditions.size(); k++) {
        const sixdof_dwell_condition& c = conditions[k];
        const sixdof_norm_probe& p = c.probe;
        const bool minus = (p.flags & kMinus) != 0;
        const int ka = column_of(p.component_id), kb = minus ? column_of(p.minus_component_id) : ka;
        for (uint64_t run = 0; run < runs; run++) {
            std::vector<PlainSample> samples;
            for (uint64_t tick : ticks) {
                const T* a = r.truth[ka][tick - 1].data() + (run * period + p.group) * kWidths[ka] + p.element;
                const T* b = r.truth[kb][tick - 1].data() + (run * period + (minus ? p.minus_group : p.group)) * kWidths[kb] + (minus ? p.minus_element : p.element);
                const double v = c.kind == kElement ? plain_element(a, b, minus) : plain_norm_sq(a, b, p.count, minus);
                samples.push_back({plain_state(v, c.op, c.lo, c.hi), tick});
            }
            const std::vector<uint64_t> w = plain_words(samples);
            for (size_t f = 0; f < kPlanes; f++) out[(k * kPlanes + f) * runs + run] = double(w[f]);
        }
    }
    return out;
}
template <class T>
std::vector<double> plain_loop(const Recorded<T>& r, const std::vector<sixdof_dwell_condition>& conditions, uint32_t period, uint64_t first, uint64_t n_samples, uint64_t every) {
    std::vector<uint64_t> ticks;
    for (uint64_t j = 0; j < n_samples; j++) ticks.push_back(first + j * every);
    return plain_loop(r, conditions, period, ticks);
}

// samples [0, n_samples) of the range in calls that begin at the sample indices `cuts` (cuts[0] = 0): the calls before the last
// hold, the second and later ones continue
template <class T>
bool read_cut(const Recorded<T>& r, const std::vector<sixdof_dwell_condition>& conditions, uint32_t period, std::vector<double>& out, uint64_t first, uint64_t n_samples,
              uint64_t every, const std::vector<uint64_t>& cuts, uint32_t last_flags = 0) {
    for (size_t c = 0; c < cuts.size(); c++) {
        const uint64_t lo = cuts[c], hi = c + 1 < cuts.size() ? cuts[c + 1] : n_samples;
        const bool last = c + 1 == cuts.size();
        const uint32_t flags = (c ? kContinue : 0u) | (last ? last_flags : kHold);
        if (sixdof_history_dwell(r.h, conditions.data(), conditions.size(), period, first + lo * every, hi - lo, every, last ? out.data() : nullptr, flags) != SIXDOF_OK) return false;
    }
    return true;
}

// what the values cases saw, over all of them: the planes must be able to go wrong
uint64_t g_max_entries = 0, g_longest_below_held = 0, g_open_start = 0, g_open_end = 0, g_counts_differ = 0, g_never = 0;

template <class T>
void values_case(uint64_t n, uint32_t period, uint64_t ring, uint64_t ticks, uint64_t first, uint64_t every, RecordOptions o) {
    Recorded<T> r(n, ring, ticks, o);
    const uint64_t n_samples = (ticks - first) / every + 1, runs = n / period;
    const std::string what = std::string(sizeof(T) == 4 ? "f32" : "f64") + " n " + std::to_string(n) + " period " + std::to_string(period) + " samples " +
                             std::to_string(n_samples) + (o.crafted_vel ? " crafted" : "");
    const uint32_t lastg = period - 1, midg = period / 2;
    const double offset = sizeof(T) == 4 ? 640.0 : 6.4e6;       // world_pos: offset plus a unit normal
    const std::vector<sixdof_dwell_condition> conditions = {
        condition(kElement, kGt, 0.0, 0.0, "world_vel", 4, 1),                                            // crafted: +-0 at a level of 0, denormals, the largest values
        condition(kElement, kInside, -3.0, 3.0, "world_vel", 5, 1, lastg),                                // crafted: NaN rows, +-inf, integers that meet both levels
        condition(kElement, kOutside, -0.5, 0.5, "world_pos", 4, 1, 0, "world_pos", 5, lastg),            // a difference of two rows of a run
        condition(kElement, kGe, 0.0, 0.0, "world_vel", 4, 1, 0, "world_vel", 4, lastg),                  // crafted: the largest minus the lowest overflows
        condition(kNormSq, kLt, 60.0, 0.0, "world_vel", 3, 3, midg),                                      // |v|^2; crafted: overflowing squares, NaN, inf
        condition(kNormSq, kGe, 3.0 * offset * offset, 0.0, "world_pos", 4, 3, lastg, "world_accel", 0, midg),   // a separation across components
        condition(kNormSq, kLe, 0.25, 0.0, "force", 4, 1, lastg),                                         // count 1; with holes: NaN at every tick
        condition(kNormSq, kOutside, 1.0, 9.0, "world_vel", 1, 2, 0, "force", 2, lastg),
    };
    force_segments(0);
    const size_t doubles = conditions.size() * kPlanes * runs;
    std::vector<double> whole(doubles, -7.0);
    if (!read_cut(r, conditions, period, whole, first, n_samples, every, {0})) return complain(what + ": " + sixdof_last_error(r.h));
    const std::vector<double> want = plain_loop(r, conditions, period, first, n_samples, every);
    for (size_t i = 0; i < doubles; i++)
        if (std::memcmp(&want[i], &whole[i], 8) != 0) {
            complain(what + ": condition " + std::to_string(i / (kPlanes * runs)) + " plane " + std::to_string(i / runs % kPlanes) + " run " + std::to_string(i % runs) + ": " +
                     std::to_string(whole[i]) + " != " + std::to_string(want[i]));
            break;
        }
    for (size_t k = 0; k < conditions.size(); k++)
        for (uint64_t run = 0; run < runs; run++) {
            const double* p = want.data() + k * kPlanes * runs + run;
            g_max_entries = std::max<uint64_t>(g_max_entries, uint64_t(p[2 * runs]));
            g_longest_below_held += p[9 * runs] < p[runs], g_open_start += p[5 * runs] > 0, g_open_end += p[7 * runs] > 0, g_never += p[0] > 0 && p[runs] == 0;
            g_counts_differ += p[0] != want[k * kPlanes * runs];
        }
    // cut-independence: the same range in 2 and in 3 calls, and under forced segment counts
    std::vector<std::vector<uint64_t>> cuttings;
    if (n_samples >= 2) cuttings.push_back({0, n_samples / 2}), cuttings.push_back({0, 1});
    if (n_samples >= 3) cuttings.push_back({0, n_samples / 3, 2 * n_samples / 3});
    for (const auto& cuts : cuttings) {
        std::vector<double> cut(doubles, -9.0);
        if (!read_cut(r, conditions, period, cut, first, n_samples, every, cuts, cuts.size() == 3 ? SIXDOF_DWELL_ASYNC : 0u) || sixdof_download_wait(r.h) != SIXDOF_OK)
            return complain(what + ": in " + std::to_string(cuts.size()) + " calls: " + sixdof_last_error(r.h));
        if (!same_bits(cut, whole)) complain(what + ": the range in " + std::to_string(cuts.size()) + " calls (second from sample " + std::to_string(cuts[1]) + ") differs from one call");
    }
    for (uint64_t segments : {uint64_t(1), uint64_t(2), uint64_t(3), uint64_t(5), n_samples, n_samples + 5}) {      // n_samples: one sample per segment
        force_segments(segments);
        std::vector<double> forced(doubles, -9.0);
        if (!read_cut(r, conditions, period, forced, first, n_samples, every, {0})) return complain(what + ": " + std::to_string(segments) + " segments: " + sixdof_last_error(r.h));
        if (!same_bits(forced, whole)) complain(what + ": " + std::to_string(segments) + " forced segments differ from the plan's choice");
        for (const auto& cuts : cuttings) {     // segments and calls together: the accumulator comes first in the merge launch
            std::vector<double> both(doubles, -9.0);
            if (!read_cut(r, conditions, period, both, first, n_samples, every, cuts) || !same_bits(both, whole))
                complain(what + ": " + std::to_string(segments) + " forced segments in " + std::to_string(cuts.size()) + " calls differ");
        }
    }
    force_segments(0);
    // one condition alone is its block of the eight
    for (size_t k : {size_t(0), conditions.size() - 1}) {
        std::vector<double> one(kPlanes * runs, -9.0);
        if (!read_cut(r, {conditions[k]}, period, one, first, n_samples, every, {0}) || std::memcmp(one.data(), whole.data() + k * kPlanes * runs, one.size() * 8) != 0)
            complain(what + ": condition " + std::to_string(k) + " alone differs");
    }
    if (sixdof_sync(r.h) != SIXDOF_OK) complain(what + ": sync");
}

// Every refusal leaves the buffer and the accumulator untouched: an accumulator over ticks 5 .. 6 is made first, and continued
// over 7 .. 10 after the refusals; the result equals one call over 5 .. 10.
void refusals() {
    Recorded<double> r(24, 6, 10);   // recording since tick 3, the ring keeps 5 .. 10
    const uint64_t inertia = sixdof_component_id("inertia");
    const sixdof_dwell_condition good = condition(kElement, kInside, -0.5, 0.5, "world_vel", 3, 1, 1, "world_accel", 4, 0);
    const sixdof_dwell_condition good_sq = condition(kNormSq, kGt, 2.0, 0.0, "world_vel", 3, 3, 1);
    const uint32_t period = 2;
    const size_t doubles = kPlanes * 12;
    std::vector<double> buf(doubles, 123.0), want(doubles, -1.0);
    auto read = [&](const sixdof_dwell_condition* c, size_t nc, uint32_t per, uint64_t first, uint64_t samples, uint64_t every, double* dst, uint32_t flags) {
        return sixdof_history_dwell(r.h, c, nc, per, first, samples, every, dst, flags);
    };
    if (read(&good, 1, period, 5, 6, 1, want.data(), 0) != SIXDOF_OK) return complain(std::string("refusals: ") + sixdof_last_error(r.h));
    if (read(&good, 1, period, 5, 2, 1, nullptr, kHold) != SIXDOF_OK) return complain(std::string("refusals: hold: ") + sixdof_last_error(r.h));
    auto expect = [&](const char* what, int rc, int status) {
        if (rc != status) complain(std::string("refusal: ") + what + ": status " + std::to_string(rc) + ", expected " + std::to_string(status));
        else if (status != SIXDOF_OK && !*sixdof_last_error(r.h)) complain(std::string("refusal: ") + what + ": no message");
        if (status != SIXDOF_OK) std::printf("refusal: %s: %s\n", what, sixdof_last_error(r.h));
        for (double v : buf)
            if (v != 123.0) return complain(std::string("refusal: ") + what + ": something was copied"), void();
    };
    auto with = [&](auto change) { sixdof_dwell_condition c = good; change(c); return c; };
    auto with_sq = [&](auto change) { sixdof_dwell_condition c = good_sq; change(c); return c; };
    auto one = [&](const sixdof_dwell_condition& c, uint32_t flags = 0) { return read(&c, 1, period, 7, 2, 1, buf.data(), flags); };
    const int bad = SIXDOF_ERR_INVALID_ARGUMENT;
    using Cond = sixdof_dwell_condition;
    // what sixdof_history_norms refuses
    expect("every = 0", read(&good, 1, period, 7, 2, 0, buf.data(), 0), bad);
    expect("fallen out of the ring", read(&good, 1, period, 4, 2, 1, buf.data(), 0), bad);
    expect("beyond tick", read(&good, 1, period, 9, 3, 1, buf.data(), 0), bad);
    expect("last sample beyond tick", read(&good, 1, period, 5, 3, 3, buf.data(), 0), bad);
    expect("unknown flags", one(good, 8u), bad);
    expect("null conditions", read(nullptr, 1, period, 7, 2, 1, buf.data(), 0), bad);
    expect("null buffer", read(&good, 1, period, 7, 2, 1, nullptr, 0), bad);
    expect("null buffer, continuing", read(&good, 1, period, 7, 2, 1, nullptr, kContinue), bad);
    expect("null conditions, held", read(nullptr, 1, period, 7, 2, 1, nullptr, kHold), bad);
    expect("no conditions", read(&good, 0, period, 7, 2, 1, buf.data(), 0), bad);
    {
        std::vector<Cond> nine(9, good);
        expect("9 conditions", read(nine.data(), 9, period, 7, 2, 1, buf.data(), 0), bad);
    }
    expect("period = 0", read(&good, 1, 0, 7, 2, 1, buf.data(), 0), bad);
    expect("period does not divide n", read(&good, 1, 7, 7, 2, 1, buf.data(), 0), bad);
    expect("count = 0", one(with([](Cond& c) { c.probe.count = 0; })), bad);
    expect("count = 5", one(with_sq([](Cond& c) { c.probe.count = 5; })), bad);
    expect("element + count above the width", one(with_sq([](Cond& c) { c.probe.element = 4; })), bad);
    expect("element above the width", one(with([](Cond& c) { c.probe.element = 6; })), bad);
    expect("minus_element above the width", one(with([](Cond& c) { c.probe.minus_element = 6; })), bad);
    expect("element far above the width", one(with([](Cond& c) { c.probe.element = 0xffffffffu; })), bad);
    expect("group = period", one(with([](Cond& c) { c.probe.group = 2; })), bad);
    expect("minus_group = period", one(with([](Cond& c) { c.probe.minus_group = 2; })), bad);
    expect("unknown probe flags", one(with([](Cond& c) { c.probe.flags = 3; })), bad);
    expect("a probe of inertia, which is not recorded", one(with([&](Cond& c) { c.probe.component_id = inertia; })), SIXDOF_ERR_COMPONENT_NOT_FOUND);
    expect("minus inertia", one(with([&](Cond& c) { c.probe.minus_component_id = inertia; })), SIXDOF_ERR_COMPONENT_NOT_FOUND);
    {
        const Cond c = with([&](Cond& q) { q.probe.minus_component_id = inertia; });
        expect("minus inertia, held", read(&c, 1, period, 7, 2, 1, nullptr, kHold), SIXDOF_ERR_COMPONENT_NOT_FOUND);
    }
    // the reader's own
    expect("unknown kind", one(with([](Cond& c) { c.kind = 2; })), bad);
    expect("unknown op", one(with([](Cond& c) { c.op = 6; })), bad);
    expect("unknown op, far", one(with([](Cond& c) { c.op = 0xffffffffu; })), bad);
    expect("count = 2 of an element", one(with([](Cond& c) { c.probe.count = 2; })), bad);
    expect("count = 3 of an element", one(with_sq([](Cond& c) { c.kind = kElement; })), bad);
    expect("lo is NaN", one(with([](Cond& c) { c.lo = kNaN; })), bad);
    expect("hi is NaN", one(with([](Cond& c) { c.hi = kNaN; })), bad);
    expect("lo is -inf", one(with([](Cond& c) { c.lo = -kInf; })), bad);
    expect("hi is inf", one(with([](Cond& c) { c.hi = kInf; })), bad);
    expect("the level of a one-sided op is inf", one(with_sq([](Cond& c) { c.lo = kInf; })), bad);
    expect("hi != 0 with <", one(with([](Cond& c) { c.op = kLt, c.lo = 0.0, c.hi = 0.5; })), bad);
    expect("hi != 0 with <=", one(with([](Cond& c) { c.op = kLe, c.hi = 0.5; })), bad);
    expect("hi != 0 with >", one(with_sq([](Cond& c) { c.hi = 3.0; })), bad);
    expect("hi != 0 with >=", one(with_sq([](Cond& c) { c.op = kGe, c.hi = -1.0; })), bad);
    expect("lo > hi inside", one(with([](Cond& c) { c.lo = 0.75; })), bad);
    expect("lo > hi outside", one(with([](Cond& c) { c.op = kOutside, c.hi = -0.75; })), bad);
    expect("a negative squared level", one(with_sq([](Cond& c) { c.lo = -2.0; })), bad);
    expect("a negative squared lo inside", one(with_sq([](Cond& c) { c.op = kInside, c.lo = -1.0, c.hi = 4.0; })), bad);
    expect("negative squared levels outside", one(with_sq([](Cond& c) { c.op = kOutside, c.lo = -4.0, c.hi = -1.0; })), bad);
    {
        const Cond two[2] = {good, with([](Cond& c) { c.op = 7; })};
        expect("the second condition's op", read(two, 2, period, 7, 2, 1, buf.data(), 0), bad);
    }
    expect("continue with another element", one(with([](Cond& c) { c.probe.element = 2; }), kContinue), bad);
    expect("continue with another lo", one(with([](Cond& c) { c.lo = -0.25; }), kContinue), bad);
    expect("continue from a tick already accumulated", read(&good, 1, period, 6, 5, 1, buf.data(), kContinue), bad);
    expect("no samples", read(&good, 1, period, 99, 0, 7, buf.data(), 0), SIXDOF_OK);
    expect("no samples, continuing", read(&good, 1, period, 99, 0, 7, buf.data(), kContinue), SIXDOF_OK);
    if (read(&good, 1, period, 7, 4, 1, buf.data(), kContinue) != SIXDOF_OK) complain(std::string("refusals: continue after them: ") + sixdof_last_error(r.h));
    if (!same_bits(buf, want)) complain("refusals: the accumulator is not what the held call left");
    std::fill(buf.begin(), buf.end(), 123.0);
    // without MINUS the three minus_ fields are not read: whatever they hold, the condition is served; lo = hi and -0.0 levels are served
    {
        Cond plain = condition(kElement, kLe, 0.0, 0.0, "world_vel", 3, 1, 1), noisy = plain;
        noisy.probe.minus_component_id = inertia, noisy.probe.minus_element = 99, noisy.probe.minus_group = 99;
        std::vector<double> a(doubles, -1.0), b(doubles, -2.0);
        if (read(&plain, 1, period, 5, 6, 1, a.data(), 0) != SIXDOF_OK || read(&noisy, 1, period, 5, 6, 1, b.data(), 0) != SIXDOF_OK || !same_bits(a, b))
            complain("refusals: the minus_ fields are read without SIXDOF_NORM_MINUS");
        const Cond point = condition(kElement, kInside, 0.25, 0.25, "world_vel", 3, 1, 1), zero = condition(kNormSq, kGe, -0.0, 0.0, "world_vel", 3, 3, 1),
                   zero_hi = condition(kElement, kGt, 1.0, -0.0, "world_vel", 3, 1, 1);
        if (read(&point, 1, period, 5, 6, 1, a.data(), 0) != SIXDOF_OK || read(&zero, 1, period, 5, 6, 1, a.data(), 0) != SIXDOF_OK || read(&zero_hi, 1, period, 5, 6, 1, a.data(), 0) != SIXDOF_OK)
            complain(std::string("refusals: lo = hi, a squared level of -0.0 or hi = -0.0 is refused: ") + sixdof_last_error(r.h));
    }
    // ticks a double cannot hold: 2^53 - 2 and 2^53 - 1 are served, 2^53 is not
    const uint64_t top = uint64_t(1) << 53;
    if (sixdof_set_tick(r.h, top - 3) != SIXDOF_OK || sixdof_step(r.h, 3, nullptr) != SIXDOF_OK) complain(std::string("refusals: stepping to 2^53: ") + sixdof_last_error(r.h));
    expect("a sampled tick of 2^53", read(&good_sq, 1, period, top - 2, 3, 1, buf.data(), 0), bad);
    {
        const Cond always = condition(kNormSq, kGe, 0.0, 0.0, "world_vel", 3, 3, 1);
        if (read(&always, 1, period, top - 2, 2, 1, buf.data(), 0) != SIXDOF_OK || buf[3 * 12] != double(top - 2) || buf[4 * 12] != double(top - 1) || buf[11 * 12] != double(top - 1))
            complain("refusals: ticks 2^53 - 2 and 2^53 - 1 are not served");
    }
    std::fill(buf.begin(), buf.end(), 123.0);
    if (sixdof_set_history(r.h, 0) != SIXDOF_OK) complain("refusal: set_history(0)");
    expect("no ring", one(good), bad);
    expect("no ring, continuing", one(good, kContinue), bad);
}

// When SIXDOF_DWELL_CONTINUE is refused and when it is accepted.
void continue_conditions() {
    Recorded<double> r(24, 8, 10);   // the ring keeps 3 .. 10
    const std::vector<sixdof_dwell_condition> conditions = {condition(kNormSq, kLt, 3.0, 0.0, "world_vel", 0, 3), condition(kElement, kInside, -0.5, 1.0, "force", 3, 1, 2, "world_accel", 1, 1)};
    const uint32_t period = 3;
    const uint64_t runs = 24 / period;
    const size_t doubles = 2 * kPlanes * runs;
    std::vector<double> out(doubles, -7.0), want(doubles, -9.0);
    using Cond = sixdof_dwell_condition;
    auto call = [&](const std::vector<Cond>& c, uint32_t per, uint64_t first, uint64_t samples, uint64_t every, std::vector<double>* to, uint32_t flags) {
        return sixdof_history_dwell(r.h, c.data(), c.size(), per, first, samples, every, to ? to->data() : nullptr, flags);
    };
    auto refused = [&](const char* what, int rc) {
        if (rc != SIXDOF_ERR_INVALID_ARGUMENT || !*sixdof_last_error(r.h)) complain(std::string("continue ") + what + ": status " + std::to_string(rc));
        else std::printf("refusal: continue %s: %s\n", what, sixdof_last_error(r.h));
        if (out[0] != -7.0 || out.back() != -7.0) complain(std::string("continue ") + what + ": something was copied");
    };
    auto changed = [&](auto change) { std::vector<Cond> c = conditions; change(c[1]); return c; };
    refused("with no accumulator", call(conditions, period, 3, 2, 1, &out, kContinue));
    if (call(conditions, period, 3, 2, 1, nullptr, kHold) != SIXDOF_OK) return complain(std::string("continue: hold: ") + sixdof_last_error(r.h));
    refused("with fewer conditions", call({conditions[0]}, period, 5, 2, 1, &out, kContinue));
    refused("with the conditions in another order", call({conditions[1], conditions[0]}, period, 5, 2, 1, &out, kContinue));
    refused("with another component", call(changed([](Cond& c) { c.probe.component_id = sixdof_component_id("world_vel"); }), period, 5, 2, 1, &out, kContinue));
    refused("with another minus component", call(changed([](Cond& c) { c.probe.minus_component_id = sixdof_component_id("world_vel"); }), period, 5, 2, 1, &out, kContinue));
    refused("with another element", call(changed([](Cond& c) { c.probe.element = 4; }), period, 5, 2, 1, &out, kContinue));
    refused("with another minus element", call(changed([](Cond& c) { c.probe.minus_element = 0; }), period, 5, 2, 1, &out, kContinue));
    refused("with another group", call(changed([](Cond& c) { c.probe.group = 1; }), period, 5, 2, 1, &out, kContinue));
    refused("with another minus group", call(changed([](Cond& c) { c.probe.minus_group = 0; }), period, 5, 2, 1, &out, kContinue));
    refused("with other probe flags", call(changed([](Cond& c) { c.probe.flags = 0; }), period, 5, 2, 1, &out, kContinue));
    refused("with another kind", call(changed([](Cond& c) { c.kind = kNormSq, c.lo = 0.5; }), period, 5, 2, 1, &out, kContinue));
    refused("with another op", call(changed([](Cond& c) { c.op = kOutside; }), period, 5, 2, 1, &out, kContinue));
    refused("with another lo", call(changed([](Cond& c) { c.lo = -0.25; }), period, 5, 2, 1, &out, kContinue));
    refused("with another hi", call(changed([](Cond& c) { c.hi = 1.5; }), period, 5, 2, 1, &out, kContinue));
    refused("with hi = -0.0 for 0.0", call({condition(kNormSq, kLt, 3.0, -0.0, "world_vel", 0, 3), conditions[1]}, period, 5, 2, 1, &out, kContinue));
    refused("with another period", call(conditions, 6, 5, 2, 1, &out, kContinue));
    refused("from the last accumulated tick", call(conditions, period, 4, 2, 1, &out, kContinue));
    // accepted after a held call, with a gap (every = 2 from tick 6): samples 3 4 6 8 10 — the plain loop over exactly those
    if (call(conditions, period, 6, 3, 2, &out, kContinue) != SIXDOF_OK) return complain(std::string("continue after hold: ") + sixdof_last_error(r.h));
    if (!same_bits(out, plain_loop(r, conditions, period, {3, 4, 6, 8, 10}))) complain("continue after hold differs from the plain loop over its samples");
    std::fill(out.begin(), out.end(), -7.0);
    // a delivered call leaves an accumulator too: continue it
    if (call(conditions, period, 3, 4, 1, &want, 0) != SIXDOF_OK || call(conditions, period, 7, 4, 1, &want, kContinue) != SIXDOF_OK || call(conditions, period, 3, 8, 1, &out, 0) != SIXDOF_OK ||
        !same_bits(out, want))
        complain("continue after a delivered call differs from one call");
    std::fill(out.begin(), out.end(), -7.0);
    // after a call that failed in the runtime: refused, and a fresh call is correct
    if (call(conditions, period, 3, 2, 1, nullptr, kHold) != SIXDOF_OK) complain("continue: second hold");
    hip_fake::fail_after(0);
    const int rc = call(conditions, period, 5, 2, 1, nullptr, kHold | kContinue);
    const bool fired = hip_fake::fired();
    hip_fake::fail_after(-1);
    if (rc != SIXDOF_ERR_BACKEND || !fired) complain("continue: the injected fault did not fail the call");
    refused("after a failed call", call(conditions, period, 7, 2, 1, &out, kContinue));
    if (call(conditions, period, 3, 8, 1, &out, 0) != SIXDOF_OK || !same_bits(out, want)) complain("continue: the fresh call after a failed one is wrong");
    std::fill(out.begin(), out.end(), -7.0);
    // the other scans keep accumulators of their own: a norms read in between does not disturb this one
    {
        const sixdof_norm_probe p = conditions[0].probe;
        std::vector<double> norms(SIXDOF_NORMS_PLANES * runs);
        if (call(conditions, period, 3, 4, 1, nullptr, kHold) != SIXDOF_OK || sixdof_history_norms(r.h, &p, 1, period, 3, 8, 1, norms.data(), 0) != SIXDOF_OK ||
            call(conditions, period, 7, 4, 1, &out, kContinue) != SIXDOF_OK || !same_bits(out, want))
            complain("continue: another scan in between disturbs the accumulator");
        // and the norms' count is this reader's: both count the samples at which the squared norm is finite
        for (uint64_t run = 0; run < runs; run++)
            if (norms[run] != out[run]) complain("continue: count differs from the norms' count");
        std::fill(out.begin(), out.end(), -7.0);
    }
    // after sixdof_set_history: the ring, and the accumulator with it, are new
    if (call(conditions, period, 3, 2, 1, nullptr, kHold) != SIXDOF_OK || sixdof_set_history(r.h, 8) != SIXDOF_OK || sixdof_step(r.h, 2, nullptr) != SIXDOF_OK)
        complain(std::string("continue: set_history: ") + sixdof_last_error(r.h));
    refused("after sixdof_set_history", call(conditions, period, 11, 2, 1, &out, kContinue));
    if (call(conditions, period, 11, 2, 1, &out, 0) != SIXDOF_OK || out[0] == -7.0) complain("continue: the fresh call on the new ring is wrong");
}

// What the fault sweep reads: ticks 4, 6, 8 — an element of world_pos, |r|^2 of it, and world_pos against force, whose element 4 is
// NaN in every row — tick 4 held, 6 and 8 continued in two segments, so that scratch, both launches and the delivery are among
// the calls that fail.  dst[0] takes the planes, dst[1] nothing.  After every run the ring is intact.
const std::vector<sixdof_dwell_condition> kSweptConditions = {condition(kElement, kGt, 6.4e6, 0.0, "world_pos", 4, 1), condition(kNormSq, kGe, 0.0, 0.0, "world_pos", 4, 3),
                                                              condition(kNormSq, kGe, 0.0, 0.0, "world_pos", 4, 3, 0, "force", 2, 0)};
const SweptRead kSwept{
    "dwell", {}, [](int k) { return k ? size_t(1) : size_t(3 * kPlanes * 40); },
    [](sixdof_handle* h, const uint64_t*, void* const dst[2], bool async) {
        const int rc = sixdof_history_dwell(h, kSweptConditions.data(), 3, 1, 4, 1, 2, nullptr, kHold);
        return rc != SIXDOF_OK ? rc : sixdof_history_dwell(h, kSweptConditions.data(), 3, 1, 6, 2, 2, static_cast<double*>(dst[0]), kContinue | (async ? SIXDOF_DWELL_ASYNC : 0u));
    },
    [](const Recorded<double>& r, bool fault_free, const std::vector<double> want[2], const std::string& run) {
        if (fault_free) {
            const std::vector<double> plain = plain_loop(r, kSweptConditions, 1, 4, 3, 2);
            if (!same_bits(want[0], plain)) complain(run + ": the values are not the plain loop's");
            // |r|^2 >= 0 holds at all three samples: one stretch from tick 4 to tick 8; against force no sample is finite
            if (plain[kPlanes * 40] != 3.0 || plain[(kPlanes + 1) * 40] != 3.0 || plain[(kPlanes + 2) * 40] != 1.0 || plain[(kPlanes + 10) * 40] != 4.0 ||
                plain[(kPlanes + 11) * 40] != 8.0 || plain[2 * kPlanes * 40] != 0.0)
                complain(run + ": the swept read does not see what it was made to see");
        }
        std::vector<double> block(40 * 7);   // tick 9 of world_pos is what was uploaded before it
        if (sixdof_history_read(r.h, sixdof_component_id("world_pos"), 9, block.data()) != SIXDOF_OK || std::memcmp(block.data(), r.truth[0][8].data(), block.size() * 8) != 0)
            complain(run + ": the ring is not what it was");
    }};

}  // namespace

int main() {
    const RecordOptions random{}, crafted{true, true, true};
    plan_arithmetic();
    value_function<double>();
    value_function<float>();
    rule_over_cuts();
    values_case<double>(300, 4, 10, 27, 18, 3, crafted);     // the range wraps the ring (slots 7 .. 9, 0 .. 6), every third tick
    values_case<float>(300, 1, 10, 27, 18, 3, crafted);
    values_case<double>(300, 1, 8, 9, 3, 1, crafted);        // every recorded tick: the crafted block rotates through 7 ticks
    values_case<float>(300, 3, 8, 9, 3, 1, crafted);         // three rows per run
    values_case<double>(4099, 1, 4, 5, 3, 2, random);        // a ragged last block
    values_case<float>(64, 4, 8, 8, 3, 1, random);
    values_case<double>(260, 4, 40, 42, 3, 1, random);       // 40 samples, 65 runs: one past a wavefront; the plan cuts them itself
    values_case<double>(514, 2, 40, 42, 30, 1, crafted);     // 13 samples: no multiple of a load depth nor of the segment counts; 257 runs
    values_case<float>(130, 2, 40, 70, 31, 1, random);       // 40 samples out of a ring that has wrapped
    values_case<double>(2, 2, 4, 4, 4, 1, random);           // one run, one sample
    values_case<double>(65, 1, 4, 4, 4, 1, crafted);         // one sample
    if (g_max_entries < 3 || !g_longest_below_held || !g_open_start || !g_open_end || !g_counts_differ || !g_never)
        complain("values: the cases never saw three stretches, a longest below held, an open start or end, differing counts or a condition that never held");
    refusals();
    continue_conditions();
    force_segments(2);
    failure_injection("dwell_host_test", kSwept, {true, false, true});
    failure_injection("dwell_host_test", kSwept, {true, false, true}, hip_fake::kComputeFirst);
    force_segments(0);
    return verdict("dwell_host_test");
}
