// norm_events_host_test.cpp — sixdof_history_norm_events (sixdof_capi.cpp) over the fake runtime (hip_fake.cpp), whose launcher walks
// and merges through norm_events_plan.hpp — norm_events_walk, the function the kernel calls: the norms' value and walk under the
// events' rule — in the kernels' time segments, and captures through the events' capture, under AddressSanitizer / UBSan and
// without FMA contraction, no GPU: `make norm_events_test`, tests/test_history_norm_events_host.py.
//
// The ring and the fault sweep are ring_host_fixture.hpp's.  Checked: the rule over every cut of random and crafted sequences of
// squared norms into 2 and 3 parts, against one walk and against a plain loop, all four ops, both modes; every plane and capture
// bitwise against a plain loop over the fixture's host copy of the ring — count 1 to 4, with and without MINUS, f64 and f32, +-0,
// denormals, NaN, +-inf and squares that overflow, period 1 to 4, ranges that wrap the ring, take every k-th tick or hold one
// sample; one call against the same range in 2 and 3 calls (SIXDOF_NORM_EVENTS_HOLD, then SIXDOF_NORM_EVENTS_CONTINUE) and under
// forced segment counts whose segments are shorter than, equal to and longer than each load depth; every refusal with nothing
// copied and the accumulator untouched; the conditions of SIXDOF_NORM_EVENTS_CONTINUE, a level that differs in one bit among them;
// every fallible runtime call failed once.
#include "norm_events_plan.hpp"
#include "ring_host_fixture.hpp"

namespace {

constexpr size_t kPlanes = SIXDOF_NORM_EVENTS_PLANES;
constexpr uint32_t kHold = SIXDOF_NORM_EVENTS_HOLD, kContinue = SIXDOF_NORM_EVENTS_CONTINUE, kMinus = SIXDOF_NORM_MINUS;
constexpr uint32_t kLevel = SIXDOF_EVENT_LEVEL, kCrossing = SIXDOF_EVENT_CROSSING;
constexpr uint32_t kLt = SIXDOF_EVENT_LT, kLe = SIXDOF_EVENT_LE, kGt = SIXDOF_EVENT_GT, kGe = SIXDOF_EVENT_GE;

void force_segments(uint64_t count) { force_segments("SIXDOF_NORM_EVENTS_SEGMENTS", count); }
const double kNaN = std::numeric_limits<double>::quiet_NaN();
const double kInf = std::numeric_limits<double>::infinity();

// ---- the plain statements: the issue's words, one element and one sample after the other --------------------------------------
template <class T>
double plain_value(const T* a, const T* b, uint32_t count, bool minus) {
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
bool compare(double s, uint32_t op, double level_sq) {
    switch (op) {
    case SIXDOF_EVENT_LT: return s < level_sq;
    case SIXDOF_EVENT_LE: return s <= level_sq;
    case SIXDOF_EVENT_GT: return s > level_sq;
    default: return s >= level_sq;
    }
}
struct Found { uint64_t tick = 0, before = 0; double value = kNaN, value_before = kNaN; };
struct Walker {
    uint32_t op, mode;
    double level_sq;
    bool any = false, prev_holds = false;
    uint64_t prev_tick = 0;
    double prev = kNaN;
    Found f;
    void sample(uint64_t tick, double s) {
        if (!std::isfinite(s) || f.tick) return;       // skipped as if not sampled; the first event only
        const bool holds = compare(s, op, level_sq);
        const bool fires = mode == kLevel ? holds : holds && any && !prev_holds;
        if (fires) {
            f.tick = tick, f.value = s;
            if (any) f.before = prev_tick, f.value_before = prev;
            return;
        }
        any = true, prev_holds = holds, prev_tick = tick, prev = s;
    }
    void planes(double* out, size_t stride) const { out[0] = double(f.tick), out[stride] = f.value, out[2 * stride] = double(f.before), out[3 * stride] = f.value_before; }
};

// ---- the rule over every cut ---------------------------------------------------------------------------------------------
void rule_over_cuts() {
    using namespace sixdof;
    std::mt19937_64 rng(11);
    std::vector<std::vector<double>> sequences = {
        {}, {0.0}, {kNaN}, {4.0}, {0.0, 0.0, 0.0, 0.0}, {kNaN, kInf, kNaN}, {4.0, 4.0, 4.0}, {1.0, 4.0, 1.0, 4.0}, {4.0, 1.0, 4.0, 1.0, 4.0}, {kInf, 1.0, kNaN, kInf, 4.0, 1.0},
        {1.0, kNaN, 4.0}, {4.0, kInf, 1.0, kNaN, 4.0}, {5e-324, 0.0, 5e-324, 1.7e308, 1.7e308}, {1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0}, {7.0, 6.0, 5.0, 4.0, 3.0, 2.0, 1.0},
        {kNaN, kNaN, kNaN, 2.0, kNaN, 2.0, 4.0, kNaN, 4.0, 2.0, 4.0}};
    for (int k = 0; k < 200; k++) {
        std::vector<double> s(rng() % 12);
        for (double& x : s) {
            const uint64_t pick = rng() % 10;
            x = pick == 0 ? kNaN : pick == 1 ? kInf : double(rng() % 5);      // few distinct values: the level is met often, ties everywhere
        }
        sequences.push_back(s);
    }
    uint64_t checked = 0;
    for (const auto& s : sequences) {
        const uint32_t len = static_cast<uint32_t>(s.size());
        for (uint32_t op : {kLt, kLe, kGt, kGe})
            for (double level_sq : {2.0, 0.0, 4.0}) {
                auto walk = [&](uint32_t lo, uint32_t hi) {
                    EventsRecord r = events_empty();
                    for (uint32_t j = lo; j < hi; j++) norm_events_sample(r, s[j], 10 + 3 * j, op, level_sq);
                    return r;
                };
                const EventsRecord whole = walk(0, len);
                for (uint32_t mode : {kLevel, kCrossing}) {
                    Walker w{op, mode, level_sq};
                    for (uint32_t j = 0; j < len; j++) w.sample(10 + 3 * j, s[j]);
                    double want[kPlanes], got[kPlanes];
                    w.planes(want, 1);
                    events_emit<double>(whole, mode, got, 1);
                    if (std::memcmp(want, got, sizeof(got)) != 0) return complain("rule: a sequence of length " + std::to_string(len) + " differs from the plain loop");
                    auto check = [&](const EventsRecord& merged, const char* what) {
                        double planes[kPlanes];
                        events_emit<double>(merged, mode, planes, 1);
                        if (std::memcmp(planes, want, sizeof(planes)) != 0) complain(std::string("rule: ") + what + " of a sequence of length " + std::to_string(len) + " differs from one walk");
                        checked++;
                    };
                    for (uint32_t c1 = 0; c1 <= len; c1++) {
                        check(events_merge(walk(0, c1), walk(c1, len)), "a cut in 2");
                        for (uint32_t c2 = c1; c2 <= len; c2++) {
                            check(events_merge(events_merge(walk(0, c1), walk(c1, c2)), walk(c2, len)), "a cut in 3, left first");
                            check(events_merge(walk(0, c1), events_merge(walk(c1, c2), walk(c2, len))), "a cut in 3, right first");
                        }
                    }
                }
            }
    }
    // the record keeps the raw bits of the double it was handed
    {
        EventsRecord r = events_empty();
        const double a = 0.1 * 0.1, b = 3.0000000000000004;
        norm_events_sample(r, a, 5, kGe, 1.0), norm_events_sample(r, b, 6, kGe, 1.0);
        uint64_t ua, ub;
        std::memcpy(&ua, &a, 8), std::memcpy(&ub, &b, 8);
        if (r.event_tick != 6 || r.event_bits != ub || r.before_tick != 5 || r.before_bits != ua) complain("rule: the record does not keep the raw bits of s");
    }
    std::printf("norm_events_host_test: %llu merges of every cut in 2 and 3 agree with one walk\n", static_cast<unsigned long long>(checked));
}

void plan_arithmetic() {
    using namespace sixdof;
    static_assert(sizeof(sixdof_norm_trigger) == 56 && offsetof(sixdof_norm_trigger, level_sq) == 40 && offsetof(sixdof_norm_trigger, op) == 48 &&
                      offsetof(sixdof_norm_trigger, mode) == 52,
                  "sixdof_norm_trigger");
    static_assert(kNormEventsPlanes == SIXDOF_NORM_EVENTS_PLANES && kNormEventsMaxTriggers == SIXDOF_NORM_EVENTS_MAX_TRIGGERS && kNormEventsFields == 10, "constants");
    if (norm_events_segments(65536, 1024) != 1 || norm_events_segments(kNormEventsFillThreads, 1024) != 1 || norm_events_segments(1024, 8) != 1 ||
        norm_events_segments(0, 100) != 1 || norm_events_segments(1024, 1024) != (kNormEventsFillThreads + 1023) / 1024)
        complain("plan: norm_events_segments");
    for (uint64_t units : {uint64_t(1), uint64_t(125), uint64_t(7168), uint64_t(65535)})
        for (uint64_t ns : {uint64_t(1), uint64_t(13), uint64_t(64), uint64_t(1024), uint64_t(1) << 31}) {
            const uint32_t s = norm_events_segments(units, ns);
            if (s < 1 || s > ns || s > kScanMaxSegments) complain("plan: norm_events_segments out of range");
        }
    if (norm_events_record_index(2, 10, 4) != 2 * 10 * 10 + 4 || norm_events_scratch_index(2, 3, 1, 10, 4) != (2 * 3 + 1) * 10 * 10 + 4 || norm_events_out_index(2, 10, 4) != 2 * 4 * 10 + 4)
        complain("plan: indices");
    NormEventsArgs a{};
    int dummy = 0;
    a.t[0] = {{&dummy, &dummy, 7, 6, 4, 3, 3, 0, 3, kNormMinus}, 2.5, kEventGe, kEventCrossing};
    auto ok = [&] { return norm_events_launch_ok(a, 1, 8, 4, 1, 10, 1, 2); };
    if (!ok()) complain("plan: norm_events_launch_ok refuses a good launch");
    const NormEventsArgs good = a;
    a.t[0].probe.element_a = 5; if (ok()) complain("plan: element"); a = good;
    a.t[0].probe.element_b = 4; if (ok()) complain("plan: minus element"); a = good;
    a.t[0].probe.group_a = 4; if (ok()) complain("plan: group"); a = good;
    a.t[0].probe.group_b = 4; if (ok()) complain("plan: minus group"); a = good;
    a.t[0].probe.count = 0; if (ok()) complain("plan: count 0"); a = good;
    a.t[0].probe.count = 5; if (ok()) complain("plan: count 5"); a = good;
    a.t[0].probe.flags = 2; if (ok()) complain("plan: flags"); a = good;
    a.t[0].probe.ring_b = nullptr; if (ok()) complain("plan: null ring"); a = good;
    a.t[0].op = 4; if (ok()) complain("plan: op"); a = good;
    a.t[0].mode = 2; if (ok()) complain("plan: mode"); a = good;
    a.t[0].level_sq = kNaN; if (ok()) complain("plan: NaN level"); a = good;
    a.t[0].level_sq = kInf; if (ok()) complain("plan: infinite level"); a = good;
    a.t[0].level_sq = -1e-300; if (ok()) complain("plan: negative level"); a = good;
    a.t[0].level_sq = 0.0; if (!ok()) complain("plan: a level of 0 is refused"); a = good;
    if (norm_events_launch_ok(a, 0, 8, 4, 1, 10, 1, 2) || norm_events_launch_ok(a, 9, 8, 4, 1, 10, 1, 2) || norm_events_launch_ok(a, 1, 9, 4, 1, 10, 1, 2) ||
        norm_events_launch_ok(a, 1, 8, 0, 1, 10, 1, 2) || norm_events_launch_ok(a, 1, 8, 4, 1, 10, 1, 11) || norm_events_launch_ok(a, 1, 8, 4, 1, 10, 1, 0) ||
        norm_events_launch_ok(a, 1, 8, 4, uint64_t(1) << 53, 1, 1, 1))
        complain("plan: norm_events_launch_ok accepts a bad launch");
    // what the capture stage is handed passes the capture's own check and carries the modes
    const EventsArgs modes = norm_events_capture_args(good, 1);
    const uint32_t widths[1] = {7};
    if (!events_capture_ok(modes, 1, 1, 4, widths, 8, 4, 1, 10, 1) || modes.t[0].mode != kEventCrossing) complain("plan: norm_events_capture_args");
}

// ---- reads over the fixture's ring ----------------------------------------------------------------------------------------
int column_of(uint64_t id) {
    for (int k = 0; k < 4; k++)
        if (id == sixdof_component_id(kNames[k])) return k;
    return -1;
}
sixdof_norm_probe probe(const char* name, uint32_t element, uint32_t count, uint32_t group = 0) {
    sixdof_norm_probe p{};
    p.component_id = sixdof_component_id(name), p.element = element, p.count = count, p.group = group;
    return p;
}
sixdof_norm_probe probe(const char* name, uint32_t element, uint32_t count, uint32_t group, const char* minus, uint32_t minus_element, uint32_t minus_group) {
    sixdof_norm_probe p = probe(name, element, count, group);
    p.flags = kMinus, p.minus_component_id = sixdof_component_id(minus), p.minus_element = minus_element, p.minus_group = minus_group;
    return p;
}
sixdof_norm_trigger trigger(const sixdof_norm_probe& p, uint32_t op, uint32_t mode, double level_sq) {
    sixdof_norm_trigger t{};
    t.probe = p, t.level_sq = level_sq, t.op = op, t.mode = mode;
    return t;
}

// What one read returns: the event planes and one buffer per captured component.
struct Result {
    std::vector<double> events;
    std::vector<std::vector<double>> captures;
    std::vector<double*> dst;
    Result(size_t n_triggers, const std::vector<uint64_t>& cap, uint64_t n, uint32_t period, double fill = -7.0) : events(n_triggers * kPlanes * (n / period), fill) {
        for (uint64_t id : cap) captures.emplace_back(n_triggers * n * kWidths[column_of(id)], fill);
        for (auto& c : captures) dst.push_back(c.data());
    }
    bool same(const Result& o) const {
        if (!same_bits(events, o.events) || captures.size() != o.captures.size()) return false;
        for (size_t k = 0; k < captures.size(); k++)
            if (!same_bits(captures[k], o.captures[k])) return false;
        return true;
    }
};

template <class T>
Result plain_loop(const Recorded<T>& r, const std::vector<sixdof_norm_trigger>& trig, const std::vector<uint64_t>& cap, uint32_t period, const std::vector<uint64_t>& ticks) {
    Result out(trig.size(), cap, r.n, period, kNaN);
    const uint64_t runs = r.n / period;
    for (size_t t = 0; t < trig.size(); t++) {
        const sixdof_norm_probe& p = trig[t].probe;
        const bool minus = (p.flags & kMinus) != 0;
        const int ka = column_of(p.component_id), kb = minus ? column_of(p.minus_component_id) : ka;
        for (uint64_t run = 0; run < runs; run++) {
            Walker w{trig[t].op, trig[t].mode, trig[t].level_sq};
            for (uint64_t tick : ticks) {
                const T* a = r.truth[ka][tick - 1].data() + (run * period + p.group) * kWidths[ka] + p.element;
                const T* b = r.truth[kb][tick - 1].data() + (run * period + (minus ? p.minus_group : p.group)) * kWidths[kb] + (minus ? p.minus_element : p.element);
                w.sample(tick, plain_value(a, b, p.count, minus));
            }
            w.planes(out.events.data() + (t * kPlanes) * runs + run, runs);
            for (size_t c = 0; c < cap.size(); c++) {
                const int ck = column_of(cap[c]);
                const uint64_t rw = period * kWidths[ck], total = r.n * kWidths[ck];
                for (uint64_t i = run * rw; i < (run + 1) * rw; i++) out.captures[c][t * total + i] = w.f.tick ? double(r.truth[ck][w.f.tick - 1][i]) : kNaN;
            }
        }
    }
    return out;
}
template <class T>
Result plain_loop(const Recorded<T>& r, const std::vector<sixdof_norm_trigger>& trig, const std::vector<uint64_t>& cap, uint32_t period, uint64_t first, uint64_t n_samples,
                  uint64_t every) {
    std::vector<uint64_t> ticks;
    for (uint64_t j = 0; j < n_samples; j++) ticks.push_back(first + j * every);
    return plain_loop(r, trig, cap, period, ticks);
}

// samples [0, n_samples) of the range in calls that begin at the sample indices `cuts` (cuts[0] = 0): the calls before the last
// hold, the second and later ones continue
template <class T>
bool read_cut(const Recorded<T>& r, const std::vector<sixdof_norm_trigger>& trig, const std::vector<uint64_t>& cap, uint32_t period, Result& out, uint64_t first,
              uint64_t n_samples, uint64_t every, const std::vector<uint64_t>& cuts, uint32_t last_flags = 0) {
    for (size_t c = 0; c < cuts.size(); c++) {
        const uint64_t lo = cuts[c], hi = c + 1 < cuts.size() ? cuts[c + 1] : n_samples;
        const bool last = c + 1 == cuts.size();
        const uint32_t flags = (c ? kContinue : 0u) | (last ? last_flags : kHold);
        if (sixdof_history_norm_events(r.h, trig.data(), trig.size(), cap.data(), cap.size(), period, first + lo * every, hi - lo, every, last ? out.events.data() : nullptr,
                                       last ? out.dst.data() : nullptr, flags) != SIXDOF_OK)
            return false;
    }
    return true;
}

template <class T>
void values_case(uint64_t n, uint32_t period, uint64_t ring, uint64_t ticks, uint64_t first, uint64_t every, RecordOptions o) {
    Recorded<T> r(n, ring, ticks, o);
    const uint64_t n_samples = (ticks - first) / every + 1, runs = n / period;
    const std::string what = std::string(sizeof(T) == 4 ? "f32" : "f64") + " n " + std::to_string(n) + " period " + std::to_string(period) + " samples " +
                             std::to_string(n_samples) + (o.crafted_vel ? " crafted" : "");
    const uint32_t lastg = period - 1, midg = period / 2;
    const double pos0 = sizeof(T) == 4 ? 640.0 : 6.4e6;
    const std::vector<sixdof_norm_trigger> trig = {
        // |v|; crafted: +-0, denormals, the largest values (f64: their squares overflow and are skipped), NaN rows, +-inf
        trigger(probe("world_vel", 3, 3), kGe, kCrossing, 100.0),
        trigger(probe("world_pos", 4, 3, 0, "world_pos", 4, lastg), kLt, kCrossing, 4.0),     // a separation of two rows of a run; period 1: +0.0 at every tick
        trigger(probe("world_pos", 4, 3, lastg, "world_accel", 0, midg), kGt, kLevel, 3.0 * pos0 * pos0),   // across components, depth 2
        trigger(probe("world_pos", 0, 4, midg), kLe, kCrossing, 4.0 * pos0 * pos0),           // the quaternion
        trigger(probe("force", 4, 1, lastg), kGt, kLevel, 0.5),                               // count 1; with holes: NaN at every tick, no event
        trigger(probe("world_vel", 1, 2, 0, "force", 2, lastg), kGe, kCrossing, 4.0),
        trigger(probe("world_vel", 4, 1, midg), kLe, kLevel, 0.0),                            // crafted: the squares of +-0 and of the denormals are +0.0
        trigger(probe("world_accel", 0, 1, 0, "world_accel", 5, 0), kLt, kCrossing, 1.0),     // two elements of one row
    };
    const std::vector<uint64_t> cap = {sixdof_component_id("world_pos"), sixdof_component_id("world_vel")};
    force_segments(0);
    Result whole(trig.size(), cap, n, period);
    if (!read_cut(r, trig, cap, period, whole, first, n_samples, every, {0})) return complain(what + ": " + sixdof_last_error(r.h));
    const Result want = plain_loop(r, trig, cap, period, first, n_samples, every);
    for (size_t i = 0; i < want.events.size(); i++)
        if (std::memcmp(&want.events[i], &whole.events[i], 8) != 0) {
            complain(what + ": trigger " + std::to_string(i / (kPlanes * runs)) + " plane " + std::to_string(i / runs % kPlanes) + " run " + std::to_string(i % runs) + ": " +
                     std::to_string(whole.events[i]) + " != " + std::to_string(want.events[i]));
            break;
        }
    for (size_t c = 0; c < cap.size(); c++)
        if (!same_bits(want.captures[c], whole.captures[c])) complain(what + ": capture " + std::to_string(c) + " differs from the plain loop");
    // cut-independence: the same range in 2 and in 3 calls, at a cut placed on a crossing, and under forced segment counts
    std::vector<std::vector<uint64_t>> cuttings;
    if (n_samples >= 2) cuttings.push_back({0, n_samples / 2}), cuttings.push_back({0, 1});
    if (n_samples >= 3) cuttings.push_back({0, n_samples / 3, 2 * n_samples / 3});
    uint64_t crossing_cut = 0;   // the sample index of the earliest crossing that has a "before" sample in the range
    for (size_t t = 0; t < trig.size() && n_samples >= 2; t++)
        for (uint64_t run = 0; run < runs; run++) {
            const double tick = want.events[(t * kPlanes) * runs + run], before = want.events[(t * kPlanes + 2) * runs + run];
            if (before != 0 && (crossing_cut == 0 || (uint64_t(tick) - first) / every < crossing_cut)) crossing_cut = (uint64_t(tick) - first) / every;
        }
    if (crossing_cut) cuttings.push_back({0, crossing_cut});
    else if (n_samples >= 8 && runs >= 8) complain(what + ": no crossing to cut at");
    for (const auto& cuts : cuttings) {
        Result cut(trig.size(), cap, n, period, -9.0);
        if (!read_cut(r, trig, cap, period, cut, first, n_samples, every, cuts, cuts.size() == 3 ? SIXDOF_NORM_EVENTS_ASYNC : 0u) || sixdof_download_wait(r.h) != SIXDOF_OK)
            return complain(what + ": in " + std::to_string(cuts.size()) + " calls: " + sixdof_last_error(r.h));
        if (!cut.same(whole)) complain(what + ": the range in " + std::to_string(cuts.size()) + " calls (second from sample " + std::to_string(cuts[1]) + ") differs from one call");
    }
    // segments of 1 to 5 samples are shorter than, equal to and longer than the load depths 2 and 4; then one sample per segment and more than that
    std::vector<uint64_t> counts = {1, 2, 3, 5, n_samples, n_samples + 5};
    for (uint64_t len = 1; len <= 5; len++) counts.push_back(std::max<uint64_t>(1, n_samples / len));
    for (uint64_t segments : counts) {
        force_segments(segments);
        Result forced(trig.size(), cap, n, period, -9.0);
        if (!read_cut(r, trig, cap, period, forced, first, n_samples, every, {0})) return complain(what + ": " + std::to_string(segments) + " segments: " + sixdof_last_error(r.h));
        if (!forced.same(whole)) complain(what + ": " + std::to_string(segments) + " forced segments differ from the plan's choice");
        for (const auto& cuts : cuttings) {     // segments and calls together: the accumulator comes first in the merge launch
            Result both(trig.size(), cap, n, period, -9.0);
            if (!read_cut(r, trig, cap, period, both, first, n_samples, every, cuts) || !both.same(whole))
                complain(what + ": " + std::to_string(segments) + " forced segments in " + std::to_string(cuts.size()) + " calls differ");
        }
    }
    force_segments(0);
    // events only: no captures; and one trigger alone is its block of the eight
    Result bare(trig.size(), {}, n, period, -9.0);
    if (!read_cut(r, trig, {}, period, bare, first, n_samples, every, {0}) || !same_bits(bare.events, whole.events)) complain(what + ": n_captures = 0 differs");
    for (size_t k : {size_t(0), trig.size() - 1}) {
        Result one(1, {}, n, period, -9.0);
        if (!read_cut(r, {trig[k]}, {}, period, one, first, n_samples, every, {0}) || std::memcmp(one.events.data(), whole.events.data() + k * kPlanes * runs, one.events.size() * 8) != 0)
            complain(what + ": trigger " + std::to_string(k) + " alone differs");
    }
    // what the case was made to see
    if (o.holes)
        for (uint64_t run = 0; run < runs; run++)
            if (whole.events[(4 * kPlanes) * runs + run] != 0 || !std::isnan(whole.events[(4 * kPlanes + 1) * runs + run])) return complain(what + ": a run with no finite sample has an event");
    if (period == 1 && n_samples >= 2)      // a row against itself: +0.0 < 4 from the first sample on — a crossing never fires
        for (uint64_t run = 0; run < runs; run++)
            if (whole.events[(1 * kPlanes) * runs + run] != 0) return complain(what + ": a predicate that holds throughout fired as a crossing");
    if (sixdof_sync(r.h) != SIXDOF_OK) complain(what + ": sync");
}

// An overflowing square is skipped: it neither holds nor fails and is never a "before" sample.  One f64 row whose |v| is 1, then
// 1e200 (its square is +inf), then 3: s >= 4 as a crossing fires at the third sample with the first as "before"; as a LEVEL of
// s > 1e300 it never fires although +inf > 1e300.
void overflow_is_skipped() {
    Recorded<double> r(2, 4, 3);                  // recording since tick 3; ticks 4, 5 and 6 are uploaded by hand
    const double speeds[3] = {1.0, 1e200, 3.0};
    for (int t = 0; t < 3; t++) {
        for (uint64_t i = 0; i < 2 * 6; i++) r.col[1][i] = 0.0;
        r.col[1][3] = speeds[t], r.col[1][6 + 3] = speeds[t];
        if (sixdof_upload(r.h) != SIXDOF_OK || sixdof_step(r.h, 1, nullptr) != SIXDOF_OK) return complain(std::string("overflow: ") + sixdof_last_error(r.h));
    }
    const std::vector<sixdof_norm_trigger> trig = {trigger(probe("world_vel", 3, 3), kGe, kCrossing, 4.0), trigger(probe("world_vel", 3, 3), kGt, kLevel, 1e300),
                                                   trigger(probe("world_vel", 3, 1, 0, "world_vel", 0, 0), kGe, kLevel, 0.0)};
    std::vector<double> ev(3 * kPlanes * 2, -7.0);
    if (sixdof_history_norm_events(r.h, trig.data(), 3, nullptr, 0, 1, 4, 3, 1, ev.data(), nullptr, 0) != SIXDOF_OK) return complain(std::string("overflow: ") + sixdof_last_error(r.h));
    const double* a = ev.data();
    if (a[0] != 6.0 || a[2] != 9.0 || a[4] != 4.0 || a[6] != 1.0) complain("overflow: the overflowing sample was not skipped by the crossing");
    const double* b = ev.data() + kPlanes * 2;
    if (b[0] != 0.0 || !std::isnan(b[2]) || b[4] != 0.0 || !std::isnan(b[6])) complain("overflow: an infinite square held");
    const double* c = ev.data() + 2 * kPlanes * 2;   // |1e200 - 0|^2 overflows too; the first sample is the LEVEL event, nothing before
    if (c[0] != 4.0 || c[2] != 1.0 || c[4] != 0.0) complain("overflow: the level event of the separation");
}

// Every refusal leaves the buffers and the accumulator untouched: an accumulator over ticks 5 .. 6 is made first, and continued
// over 7 .. 10 after the refusals; the result equals one call over 5 .. 10.
void refusals() {
    Recorded<double> r(24, 6, 10);   // recording since tick 3, the ring keeps 5 .. 10
    const uint64_t pos = sixdof_component_id("world_pos"), vel = sixdof_component_id("world_vel"), inertia = sixdof_component_id("inertia");
    const sixdof_norm_trigger good = trigger(probe("world_vel", 3, 3, 1, "world_accel", 2, 0), kGt, kCrossing, 6.0);
    const uint32_t period = 2;
    const size_t n_ev = kPlanes * 12, n_cap = 24 * 7;
    std::vector<double> ev(n_ev, 123.0), cap(n_cap, 123.0), want_ev(n_ev, -1.0), want_cap(n_cap, -1.0);
    double* dst[1] = {cap.data()};
    double* wdst[1] = {want_cap.data()};
    double* null_dst[1] = {nullptr};
    auto read = [&](const sixdof_norm_trigger* t, size_t nt, const uint64_t* ids, size_t nc, uint32_t p, uint64_t first, uint64_t samples, uint64_t every, double* e,
                    double* const* d, uint32_t flags) { return sixdof_history_norm_events(r.h, t, nt, ids, nc, p, first, samples, every, e, d, flags); };
    if (read(&good, 1, &pos, 1, period, 5, 6, 1, want_ev.data(), wdst, 0) != SIXDOF_OK) return complain(std::string("refusals: ") + sixdof_last_error(r.h));
    if (read(&good, 1, &pos, 1, period, 5, 2, 1, nullptr, nullptr, kHold) != SIXDOF_OK) return complain(std::string("refusals: hold: ") + sixdof_last_error(r.h));
    auto expect = [&](const char* what, int rc, int status) {
        if (rc != status) complain(std::string("refusal: ") + what + ": status " + std::to_string(rc) + ", expected " + std::to_string(status));
        else if (status != SIXDOF_OK && !*sixdof_last_error(r.h)) complain(std::string("refusal: ") + what + ": no message");
        if (status != SIXDOF_OK) std::printf("refusal: %s: %s\n", what, sixdof_last_error(r.h));
        for (const auto* buf : {&ev, &cap})
            for (double v : *buf)
                if (v != 123.0) return complain(std::string("refusal: ") + what + ": something was copied"), void();
    };
    auto with = [&](auto change) { sixdof_norm_trigger t = good; change(t); return t; };
    auto one = [&](const sixdof_norm_trigger& t, uint32_t flags = 0) { return read(&t, 1, &pos, 1, period, 7, 2, 1, ev.data(), dst, flags); };
    const int bad = SIXDOF_ERR_INVALID_ARGUMENT;
    // the events' part
    expect("every = 0", read(&good, 1, &pos, 1, period, 7, 2, 0, ev.data(), dst, 0), bad);
    expect("fallen out of the ring", read(&good, 1, &pos, 1, period, 4, 2, 1, ev.data(), dst, 0), bad);
    expect("beyond tick", read(&good, 1, &pos, 1, period, 9, 3, 1, ev.data(), dst, 0), bad);
    expect("last sample beyond tick", read(&good, 1, &pos, 1, period, 5, 3, 3, ev.data(), dst, 0), bad);
    expect("unknown flags", one(good, 8u), bad);
    expect("null triggers", read(nullptr, 1, &pos, 1, period, 7, 2, 1, ev.data(), dst, 0), bad);
    expect("null capture ids", read(&good, 1, nullptr, 1, period, 7, 2, 1, ev.data(), dst, 0), bad);
    expect("null event buffer", read(&good, 1, &pos, 1, period, 7, 2, 1, nullptr, dst, 0), bad);
    expect("null capture buffer", read(&good, 1, &pos, 1, period, 7, 2, 1, ev.data(), null_dst, 0), bad);
    expect("null capture buffer list", read(&good, 1, &pos, 1, period, 7, 2, 1, ev.data(), nullptr, 0), bad);
    expect("null event buffer, continuing", read(&good, 1, &pos, 1, period, 7, 2, 1, nullptr, dst, kContinue), bad);
    expect("null triggers, held", read(nullptr, 1, &pos, 1, period, 7, 2, 1, nullptr, nullptr, kHold), bad);
    expect("no triggers", read(&good, 0, &pos, 1, period, 7, 2, 1, ev.data(), dst, 0), bad);
    {
        std::vector<sixdof_norm_trigger> nine(9, good);
        expect("9 triggers", read(nine.data(), 9, &pos, 1, period, 7, 2, 1, ev.data(), dst, 0), bad);
    }
    expect("period = 0", read(&good, 1, &pos, 1, 0, 7, 2, 1, ev.data(), dst, 0), bad);
    expect("period does not divide n", read(&good, 1, &pos, 1, 7, 7, 2, 1, ev.data(), dst, 0), bad);
    expect("unknown op", one(with([](sixdof_norm_trigger& t) { t.op = 4; })), bad);
    expect("unknown mode", one(with([](sixdof_norm_trigger& t) { t.mode = 2; })), bad);
    // the level
    expect("NaN level", one(with([](sixdof_norm_trigger& t) { t.level_sq = kNaN; })), bad);
    expect("infinite level", one(with([](sixdof_norm_trigger& t) { t.level_sq = kInf; })), bad);
    expect("negative level", one(with([](sixdof_norm_trigger& t) { t.level_sq = -4.0; })), bad);
    expect("level just below 0", one(with([](sixdof_norm_trigger& t) { t.level_sq = -5e-324; })), bad);
    // the norms' part
    expect("count = 0", one(with([](sixdof_norm_trigger& t) { t.probe.count = 0; })), bad);
    expect("count = 5", one(with([](sixdof_norm_trigger& t) { t.probe.count = 5; })), bad);
    expect("element + count above the width", one(with([](sixdof_norm_trigger& t) { t.probe.element = 4; })), bad);
    expect("minus_element + count above the width", one(with([](sixdof_norm_trigger& t) { t.probe.minus_element = 4; })), bad);
    expect("element far above the width", one(with([](sixdof_norm_trigger& t) { t.probe.element = 0xffffffffu; })), bad);
    expect("group = period", one(with([](sixdof_norm_trigger& t) { t.probe.group = 2; })), bad);
    expect("minus_group = period", one(with([](sixdof_norm_trigger& t) { t.probe.minus_group = 2; })), bad);
    expect("unknown probe flags", one(with([](sixdof_norm_trigger& t) { t.probe.flags = 3; })), bad);
    expect("a probe of inertia, which is not recorded", one(with([&](sixdof_norm_trigger& t) { t.probe.component_id = inertia; })), SIXDOF_ERR_COMPONENT_NOT_FOUND);
    expect("minus inertia", one(with([&](sixdof_norm_trigger& t) { t.probe.minus_component_id = inertia; })), SIXDOF_ERR_COMPONENT_NOT_FOUND);
    expect("capture of inertia", read(&good, 1, &inertia, 1, period, 7, 2, 1, ev.data(), dst, 0), SIXDOF_ERR_COMPONENT_NOT_FOUND);
    expect("capture of inertia, held", read(&good, 1, &inertia, 1, period, 7, 2, 1, nullptr, nullptr, kHold), SIXDOF_ERR_COMPONENT_NOT_FOUND);
    // continuing
    expect("continue with another probe", one(with([](sixdof_norm_trigger& t) { t.probe.element = 2; }), kContinue), bad);
    expect("continue with another capture list", read(&good, 1, &vel, 1, period, 7, 4, 1, ev.data(), dst, kContinue), bad);
    expect("continue from a tick already accumulated", read(&good, 1, &pos, 1, period, 6, 5, 1, ev.data(), dst, kContinue), bad);
    expect("no samples", read(&good, 1, &pos, 1, period, 99, 0, 7, ev.data(), dst, 0), SIXDOF_OK);
    expect("no samples, continuing", read(&good, 1, &pos, 1, period, 99, 0, 7, ev.data(), dst, kContinue), SIXDOF_OK);
    if (read(&good, 1, &pos, 1, period, 7, 4, 1, ev.data(), dst, kContinue) != SIXDOF_OK) complain(std::string("refusals: continue after them: ") + sixdof_last_error(r.h));
    if (!same_bits(ev, want_ev) || !same_bits(cap, want_cap)) complain("refusals: the accumulator is not what the held call left");
    {
        bool any = false;
        for (size_t i = 0; i < 12; i++) any |= want_ev[i] != 0;
        if (!any) complain("refusals: no event in the read the refusals surround");
    }
    std::fill(ev.begin(), ev.end(), 123.0), std::fill(cap.begin(), cap.end(), 123.0);
    // without MINUS the three minus_ fields are not read: whatever they hold, the trigger is served
    {
        sixdof_norm_trigger plain = trigger(probe("world_vel", 3, 3, 1), kGt, kLevel, 2.0), noisy = plain;
        noisy.probe.minus_component_id = inertia, noisy.probe.minus_element = 99, noisy.probe.minus_group = 99;
        std::vector<double> a(n_ev, -1.0), b(n_ev, -2.0);
        if (read(&plain, 1, nullptr, 0, period, 5, 6, 1, a.data(), nullptr, 0) != SIXDOF_OK || read(&noisy, 1, nullptr, 0, period, 5, 6, 1, b.data(), nullptr, 0) != SIXDOF_OK || !same_bits(a, b))
            complain("refusals: the minus_ fields are read without SIXDOF_NORM_MINUS");
    }
    // ticks a double cannot hold: 2^53 - 2 and 2^53 - 1 are served, 2^53 is not
    const uint64_t top = uint64_t(1) << 53;
    const sixdof_norm_trigger always = trigger(probe("world_vel", 3, 3, 1), kGe, kLevel, 0.0);
    if (sixdof_set_tick(r.h, top - 3) != SIXDOF_OK || sixdof_step(r.h, 3, nullptr) != SIXDOF_OK) complain(std::string("refusals: stepping to 2^53: ") + sixdof_last_error(r.h));
    expect("a sampled tick of 2^53", read(&always, 1, &pos, 1, period, top - 2, 3, 1, ev.data(), dst, 0), bad);
    if (read(&always, 1, &pos, 1, period, top - 2, 2, 1, ev.data(), dst, 0) != SIXDOF_OK || ev[0] != double(top - 2)) complain("refusals: ticks 2^53 - 2 and 2^53 - 1 are not served");
    std::fill(ev.begin(), ev.end(), 123.0), std::fill(cap.begin(), cap.end(), 123.0);
    if (sixdof_set_history(r.h, 0) != SIXDOF_OK) complain("refusal: set_history(0)");
    expect("no ring", one(good), bad);
    expect("no ring, continuing", one(good, kContinue), bad);
}

// When SIXDOF_NORM_EVENTS_CONTINUE is refused and when it is accepted.
void continue_conditions() {
    Recorded<double> r(24, 8, 10);   // the ring keeps 3 .. 10
    const std::vector<sixdof_norm_trigger> trig = {trigger(probe("world_vel", 0, 3), kGt, kCrossing, 3.0),
                                                   trigger(probe("force", 3, 2, 2, "world_accel", 1, 1), kLt, kLevel, 1.0)};
    const std::vector<uint64_t> cap = {sixdof_component_id("world_vel"), sixdof_component_id("force")}, swapped = {cap[1], cap[0]};
    const uint32_t period = 3;
    Result out(2, cap, 24, period), want(2, cap, 24, period, -9.0);
    auto call = [&](const std::vector<sixdof_norm_trigger>& t, const std::vector<uint64_t>& c, uint32_t p, uint64_t first, uint64_t samples, uint64_t every, Result* to,
                    uint32_t flags) {
        return sixdof_history_norm_events(r.h, t.data(), t.size(), c.data(), c.size(), p, first, samples, every, to ? to->events.data() : nullptr, to ? to->dst.data() : nullptr, flags);
    };
    auto refused = [&](const char* what, int rc) {
        if (rc != SIXDOF_ERR_INVALID_ARGUMENT || !*sixdof_last_error(r.h)) complain(std::string("continue ") + what + ": status " + std::to_string(rc));
        else std::printf("refusal: continue %s: %s\n", what, sixdof_last_error(r.h));
        if (out.events[0] != -7.0 || out.captures[1].back() != -7.0) complain(std::string("continue ") + what + ": something was copied");
    };
    auto changed = [&](auto change) { std::vector<sixdof_norm_trigger> t = trig; change(t[1]); return t; };
    refused("with no accumulator", call(trig, cap, period, 3, 2, 1, &out, kContinue));
    if (call(trig, cap, period, 3, 2, 1, nullptr, kHold) != SIXDOF_OK) return complain(std::string("continue: hold: ") + sixdof_last_error(r.h));
    refused("with the capture list in another order", call(trig, swapped, period, 5, 2, 1, &out, kContinue));
    refused("with a shorter capture list", call(trig, {cap[0]}, period, 5, 2, 1, &out, kContinue));
    refused("with fewer triggers", call({trig[0]}, cap, period, 5, 2, 1, &out, kContinue));
    refused("with the triggers in another order", call({trig[1], trig[0]}, cap, period, 5, 2, 1, &out, kContinue));
    refused("with another component", call(changed([](sixdof_norm_trigger& t) { t.probe.component_id = sixdof_component_id("world_vel"); }), cap, period, 5, 2, 1, &out, kContinue));
    refused("with another minus component", call(changed([](sixdof_norm_trigger& t) { t.probe.minus_component_id = sixdof_component_id("world_vel"); }), cap, period, 5, 2, 1, &out, kContinue));
    refused("with another element", call(changed([](sixdof_norm_trigger& t) { t.probe.element = 4; }), cap, period, 5, 2, 1, &out, kContinue));
    refused("with another minus element", call(changed([](sixdof_norm_trigger& t) { t.probe.minus_element = 0; }), cap, period, 5, 2, 1, &out, kContinue));
    refused("with another group", call(changed([](sixdof_norm_trigger& t) { t.probe.group = 1; }), cap, period, 5, 2, 1, &out, kContinue));
    refused("with another minus group", call(changed([](sixdof_norm_trigger& t) { t.probe.minus_group = 0; }), cap, period, 5, 2, 1, &out, kContinue));
    refused("with another count", call(changed([](sixdof_norm_trigger& t) { t.probe.count = 1; }), cap, period, 5, 2, 1, &out, kContinue));
    refused("with other probe flags", call(changed([](sixdof_norm_trigger& t) { t.probe.flags = 0; }), cap, period, 5, 2, 1, &out, kContinue));
    refused("with another op", call(changed([](sixdof_norm_trigger& t) { t.op = kLe; }), cap, period, 5, 2, 1, &out, kContinue));
    refused("with another mode", call(changed([](sixdof_norm_trigger& t) { t.mode = kCrossing; }), cap, period, 5, 2, 1, &out, kContinue));
    refused("with a level that differs in one bit", call(changed([](sixdof_norm_trigger& t) { t.level_sq = std::nextafter(1.0, 2.0); }), cap, period, 5, 2, 1, &out, kContinue));
    refused("with another period", call(trig, cap, 6, 5, 2, 1, &out, kContinue));
    refused("from the last accumulated tick", call(trig, cap, period, 4, 2, 1, &out, kContinue));
    // accepted after a held call, with a gap (every = 2 from tick 6): samples 3 4 6 8 10 — the plain loop over exactly those
    if (call(trig, cap, period, 6, 3, 2, &out, kContinue) != SIXDOF_OK) return complain(std::string("continue after hold: ") + sixdof_last_error(r.h));
    if (!out.same(plain_loop(r, trig, cap, period, {3, 4, 6, 8, 10}))) complain("continue after hold differs from the plain loop over its samples");
    auto refill = [&] {
        std::fill(out.events.begin(), out.events.end(), -7.0);
        for (auto& c : out.captures) std::fill(c.begin(), c.end(), -7.0);
    };
    refill();
    // a level of -0.0 and one of +0.0 compare alike but are other bits: refused
    {
        const std::vector<sixdof_norm_trigger> zero = {trigger(probe("world_vel", 0, 3), kGt, kCrossing, 0.0)}, minus_zero = {trigger(probe("world_vel", 0, 3), kGt, kCrossing, -0.0)};
        if (call(zero, cap, period, 3, 2, 1, nullptr, kHold) != SIXDOF_OK) complain(std::string("continue: hold at level 0: ") + sixdof_last_error(r.h));
        refused("with -0.0 for +0.0", call(minus_zero, cap, period, 5, 2, 1, &out, kContinue));
    }
    // a delivered call leaves an accumulator too: continue it
    if (call(trig, cap, period, 3, 4, 1, &want, 0) != SIXDOF_OK || call(trig, cap, period, 7, 4, 1, &want, kContinue) != SIXDOF_OK || call(trig, cap, period, 3, 8, 1, &out, 0) != SIXDOF_OK ||
        !out.same(want))
        complain("continue after a delivered call differs from one call");
    refill();
    // after a call that failed in the runtime: refused, and a fresh call is correct
    if (call(trig, cap, period, 3, 2, 1, nullptr, kHold) != SIXDOF_OK) complain("continue: second hold");
    hip_fake::fail_after(0);
    const int rc = call(trig, cap, period, 5, 2, 1, nullptr, kHold | kContinue);
    const bool fired = hip_fake::fired();
    hip_fake::fail_after(-1);
    if (rc != SIXDOF_ERR_BACKEND || !fired) complain("continue: the injected fault did not fail the call");
    refused("after a failed call", call(trig, cap, period, 7, 2, 1, &out, kContinue));
    if (call(trig, cap, period, 3, 8, 1, &out, 0) != SIXDOF_OK || !out.same(want)) complain("continue: the fresh call after a failed one is wrong");
    refill();
    // the other scans keep accumulators of their own: an events read and a norms read in between do not disturb this one
    {
        const sixdof_event_trigger et{sixdof_component_id("world_vel"), 0, 0, kGt, kCrossing, 0.5};
        const sixdof_norm_probe np = probe("world_vel", 0, 3);
        std::vector<double> eev(kPlanes * 8), nrm(SIXDOF_NORMS_PLANES * 8);
        if (call(trig, cap, period, 3, 4, 1, nullptr, kHold) != SIXDOF_OK || sixdof_history_events(r.h, &et, 1, nullptr, 0, period, 3, 8, 1, eev.data(), nullptr, 0) != SIXDOF_OK ||
            sixdof_history_norms(r.h, &np, 1, period, 3, 8, 1, nrm.data(), 0) != SIXDOF_OK || call(trig, cap, period, 7, 4, 1, &out, kContinue) != SIXDOF_OK || !out.same(want))
            complain("continue: another scan in between disturbs the accumulator");
        refill();
    }
    // after sixdof_set_history: the ring, and the accumulator with it, are new
    if (call(trig, cap, period, 3, 2, 1, nullptr, kHold) != SIXDOF_OK || sixdof_set_history(r.h, 8) != SIXDOF_OK || sixdof_step(r.h, 2, nullptr) != SIXDOF_OK)
        complain(std::string("continue: set_history: ") + sixdof_last_error(r.h));
    refused("after sixdof_set_history", call(trig, cap, period, 11, 2, 1, &out, kContinue));
    if (call(trig, cap, period, 11, 2, 1, &out, 0) != SIXDOF_OK || out.events[0] == -7.0) complain("continue: the fresh call on the new ring is wrong");
}

// What the fault sweep reads: ticks 4, 6, 8 — triggers on world_pos alone and against force, a capture of force — tick 4 held, 6 and
// 8 continued in two segments, so that records, scratch, all three launches and the delivery are among the calls that fail.
// dst[0] takes the event planes, dst[1] the capture.  After every run the ring is intact.
const std::vector<sixdof_norm_trigger> kSweptTriggers = {trigger(probe("world_pos", 4, 3), kGe, kCrossing, 3.0 * 6.4e6 * 6.4e6),
                                                         trigger(probe("world_pos", 4, 3, 0, "force", 0, 0), kLt, kLevel, 3.0 * 6.4e6 * 6.4e6)};
const SweptRead kSwept{
    "norm events", {}, [](int k) { return k ? size_t(2 * 40 * 6) : size_t(2 * kPlanes * 40); },
    [](sixdof_handle* h, const uint64_t* comp, void* const dst[2], bool async) {
        const int rc = sixdof_history_norm_events(h, kSweptTriggers.data(), 2, comp + 1, 1, 1, 4, 1, 2, nullptr, nullptr, kHold);
        double* cap[1] = {static_cast<double*>(dst[1])};
        return rc != SIXDOF_OK ? rc
                               : sixdof_history_norm_events(h, kSweptTriggers.data(), 2, comp + 1, 1, 1, 6, 2, 2, static_cast<double*>(dst[0]), cap,
                                                            kContinue | (async ? SIXDOF_NORM_EVENTS_ASYNC : 0u));
    },
    [](const Recorded<double>& r, bool fault_free, const std::vector<double> want[2], const std::string& run) {
        if (fault_free) {
            const Result plain = plain_loop(r, kSweptTriggers, {sixdof_component_id("force")}, 1, 4, 3, 2);
            if (!same_bits(want[0], plain.events) || !same_bits(want[1], plain.captures[0])) complain(run + ": the values are not the plain loop's");
            bool any = false;
            for (size_t i = 0; i < 40; i++) any |= plain.events[i] != 0;
            if (!any) complain(run + ": no event in the swept read");
        }
        std::vector<double> block(40 * 7);   // tick 9 of world_pos is what was uploaded before it
        if (sixdof_history_read(r.h, sixdof_component_id("world_pos"), 9, block.data()) != SIXDOF_OK || std::memcmp(block.data(), r.truth[0][8].data(), block.size() * 8) != 0)
            complain(run + ": the ring is not what it was");
    }};

}  // namespace

int main() {
    const RecordOptions random{}, crafted{true, true, true};
    plan_arithmetic();
    rule_over_cuts();
    values_case<double>(300, 4, 10, 27, 18, 3, crafted);     // the range wraps the ring (slots 7 .. 9, 0 .. 6), every third tick
    values_case<float>(300, 1, 10, 27, 18, 3, crafted);
    values_case<double>(300, 1, 8, 9, 3, 1, crafted);        // every recorded tick: the crafted block rotates through 7 ticks
    values_case<float>(300, 3, 8, 9, 3, 1, crafted);         // three rows per run
    values_case<double>(4099, 1, 4, 5, 3, 2, random);        // a ragged last block
    values_case<float>(64, 4, 8, 8, 3, 1, random);
    values_case<double>(260, 4, 40, 42, 3, 1, random);       // 40 samples, 65 runs: one past a wavefront; the plan cuts them itself
    values_case<double>(514, 2, 40, 42, 30, 1, crafted);     // 13 samples: no multiple of a load depth nor of the segment counts; 257 runs
    values_case<double>(2, 2, 4, 4, 4, 1, random);           // one run, one sample
    values_case<double>(65, 1, 4, 4, 4, 1, crafted);         // one sample
    overflow_is_skipped();
    refusals();
    continue_conditions();
    force_segments(2);
    failure_injection("norm_events_host_test", kSwept, {true, false, true});
    failure_injection("norm_events_host_test", kSwept, {true, false, true}, hip_fake::kComputeFirst);
    force_segments(0);
    return verdict("norm_events_host_test");
}
