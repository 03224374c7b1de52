// events_host_test.cpp — sixdof_history_events (sixdof_capi.cpp) over the fake runtime (hip_fake.cpp), whose launchers walk, merge and
// capture through events_plan.hpp in the kernels' time segments and through time_scan.hpp's scan_walk, the loop the walk kernel writes out, under AddressSanitizer / UBSan, no GPU: `make events_test`,
// tests/test_history_events_host.py.
//
// The ring and the fault sweep are ring_host_fixture.hpp's.  Checked: the rule exhaustively — every sequence of up to 8 samples
// over {holds, fails, non-finite}, both modes, every cut into 2 and 3 consecutive parts, merged records against one sequential
// walk and against a plain loop written here; every plane and every capture bitwise against that plain loop over the fixture's
// host copy of the ring, f64 and f32, period 1 and 4, over random blocks and the crafted block rotated by the tick (+-0,
// denormals, +-inf, NaN rows, an element that is NaN at every tick), ranges that wrap the ring, take every k-th tick or hold one
// sample; one call against the same range in 2 and 3 calls (SIXDOF_EVENTS_HOLD, then SIXDOF_EVENTS_CONTINUE), against a cut
// placed on a crossing (its "before" sample is the last sample of the earlier call) and against forced segment counts; every
// refusal with nothing copied and the accumulator untouched; the conditions of SIXDOF_EVENTS_CONTINUE; 33 captured components;
// every fallible runtime call failed once.
#include "events_plan.hpp"
#include "ring_host_fixture.hpp"

namespace {

constexpr size_t kPlanes = SIXDOF_EVENTS_PLANES;
constexpr uint32_t kHold = SIXDOF_EVENTS_HOLD, kContinue = SIXDOF_EVENTS_CONTINUE;
constexpr uint32_t kLevel = SIXDOF_EVENT_LEVEL, kCrossing = SIXDOF_EVENT_CROSSING;

void force_segments(uint64_t count) { force_segments("SIXDOF_EVENTS_SEGMENTS", count); }
const double kNaN = std::numeric_limits<double>::quiet_NaN();

bool compare(double x, uint32_t op, double level) {
    switch (op) {
    case SIXDOF_EVENT_LT: return x < level;
    case SIXDOF_EVENT_LE: return x <= level;
    case SIXDOF_EVENT_GT: return x > level;
    default: return x >= level;
    }
}

// ---- the plain loop: the issue's words, one sample after the other ---------------------------------------------------------
struct Found { uint64_t tick = 0, before = 0; double value = kNaN, value_before = kNaN; };
struct Walker {
    uint32_t mode;
    bool any = false, prev_holds = false;
    uint64_t prev_tick = 0;
    double prev = kNaN;
    Found f;
    void sample(uint64_t tick, double x, bool finite, bool holds) {
        if (!finite || f.tick) return;                 // skipped as if not sampled; the first event only
        const bool fires = mode == kLevel ? holds : holds && any && !prev_holds;
        if (fires) {
            f.tick = tick, f.value = x;
            if (any) f.before = prev_tick, f.value_before = prev;
            return;
        }
        any = true, prev_holds = holds, prev_tick = tick, prev = x;
    }
};

// ---- the rule, exhaustively ---------------------------------------------------------------------------------------------
// symbol 0: fails, 1: holds, 2: non-finite.  The value of sample j is j + 0.5 where it fails and -(j + 0.5) where it holds, under
// the predicate x < 0; a non-finite sample is a NaN.
void rule_exhaustive() {
    using namespace sixdof;
    uint64_t checked = 0;
    for (uint32_t len = 0; len <= 8; len++) {
        uint32_t count = 1;
        for (uint32_t i = 0; i < len; i++) count *= 3;
        for (uint32_t code = 0; code < count; code++) {
            uint32_t sym[8];
            double x[8];
            for (uint32_t j = 0, c = code; j < len; j++, c /= 3) sym[j] = c % 3, x[j] = sym[j] == 2 ? kNaN : sym[j] == 1 ? -(j + 0.5) : j + 0.5;
            auto walk = [&](uint32_t lo, uint32_t hi) {
                EventsRecord r = events_empty();
                for (uint32_t j = lo; j < hi; j++) events_sample<double>(r, x[j], 10 + 3 * j, kEventLt, 0.0);
                return r;
            };
            const EventsRecord whole = walk(0, len);
            for (uint32_t mode : {kLevel, kCrossing}) {
                Walker w{mode};
                for (uint32_t j = 0; j < len; j++) w.sample(10 + 3 * j, x[j], sym[j] != 2, sym[j] == 1);
                const double want[kPlanes] = {double(w.f.tick), w.f.value, double(w.f.before), w.f.value_before};
                double got[kPlanes];
                events_emit<double>(whole, mode, got, 1);
                if (std::memcmp(got, want, sizeof(got)) != 0) return complain("rule: sequence " + std::to_string(code) + " of length " + std::to_string(len) + " differs from the plain loop");
                auto check = [&](const EventsRecord& merged, const char* what) {
                    double planes[kPlanes];
                    events_emit<double>(merged, mode, planes, 1);
                    if (std::memcmp(planes, want, sizeof(planes)) != 0)
                        complain(std::string("rule: ") + what + " of sequence " + std::to_string(code) + " of length " + std::to_string(len) + " differs from one walk");
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
            // frozen: a record that has its crossing is left bit for bit
            if (whole.event_tick) {
                EventsRecord more = whole;
                events_accumulate(more, 77, 1000, true, true), events_accumulate(more, 78, 1001, true, false), events_accumulate(more, 79, 1002, true, true);
                const EventsRecord merged = events_merge(whole, walk(0, len));
                if (std::memcmp(&more, &whole, sizeof(whole)) != 0 || std::memcmp(&merged, &whole, sizeof(whole)) != 0) complain("rule: a frozen record changed");
            }
            // the records themselves, not only the planes, do not depend on the cut (no early stop here)
            for (uint32_t c1 = 0; c1 <= len; c1++) {
                const EventsRecord m = events_merge(walk(0, c1), walk(c1, len));
                if (std::memcmp(&m, &whole, sizeof(m)) != 0) complain("rule: the merged record of sequence " + std::to_string(code) + " differs from one walk's");
            }
        }
    }
    std::printf("events_host_test: %llu merges of every sequence of up to 8 samples agree with one walk\n", static_cast<unsigned long long>(checked));
}

void plan_arithmetic() {
    using namespace sixdof;
    if (events_segments(65536, 1024) != 1 || events_segments(kEventsFillThreads, 1024) != 1 || events_segments(1024, 1024) != 16 || events_segments(100, 1024) != 64 ||
        events_segments(1024, 8) != 1 ||
        events_segments(0, 100) != 1)
        complain("plan: events_segments");
    for (uint64_t units : {uint64_t(1), uint64_t(125), uint64_t(7168), uint64_t(65535)})
        for (uint64_t ns : {uint64_t(1), uint64_t(13), uint64_t(64), uint64_t(1024), uint64_t(1) << 31}) {
            const uint32_t s = events_segments(units, ns);
            if (s < 1 || s > ns || s > kScanMaxSegments) complain("plan: events_segments out of range");
        }
    const uint64_t rec = kEventsFields * 8;
    if (scan_fit_segments(8, 1000, kEventsFields, rec * 1000 * 3) != 3 || scan_fit_segments(8, 1000, kEventsFields, rec * 1000) != 1 || scan_fit_segments(1, 1u << 30, kEventsFields, 1) != 1) complain("plan: scan_fit_segments");
    if (scan_scratch_bytes(1, 1000, kEventsFields) != 0 || scan_scratch_bytes(3, 1000, kEventsFields) != 3 * rec * 1000 || events_record_bytes(7) != 7 * rec) complain("plan: scan_scratch_bytes");
    if (!events_tick_sampled(7, 7, 13, 3) || !events_tick_sampled(13, 7, 13, 3) || events_tick_sampled(8, 7, 13, 3) || events_tick_sampled(4, 7, 13, 3) ||
        events_tick_sampled(16, 7, 13, 3) || events_tick_sampled(0, 7, 13, 3))
        complain("plan: events_tick_sampled");
    // the predicate: an IEEE compare, -0.0 equals +0.0, NaN never holds
    if (!events_holds(-0.0, kEventLe, 0.0) || !events_holds(0.0, kEventGe, -0.0) || events_holds(-0.0, kEventLt, 0.0) || events_holds(0.0, kEventGt, -0.0) ||
        events_holds(kNaN, kEventLe, 0.0) || events_holds(kNaN, kEventGe, 0.0) || !events_holds(1.0, kEventGt, 0.5) || !events_holds(-1.0, kEventLt, 0.5))
        complain("plan: events_holds");
    EventsArgs a{};
    int dummy = 0;
    a.t[0] = {&dummy, 0.5, 7, 6, 3, kEventGe, kEventCrossing, 0};
    auto ok = [&] { return events_launch_ok(a, 1, 8, 4, 1, 10, 1, 2); };
    if (!ok()) complain("plan: events_launch_ok refuses a good launch");
    EventsArgs good = a;
    a.t[0].element = 7; if (ok()) complain("plan: element"); a = good;
    a.t[0].group = 4; if (ok()) complain("plan: group"); a = good;
    a.t[0].op = 4; if (ok()) complain("plan: op"); a = good;
    a.t[0].mode = 2; if (ok()) complain("plan: mode"); a = good;
    a.t[0].level = kNaN; if (ok()) complain("plan: NaN level"); a = good;
    a.t[0].level = std::numeric_limits<double>::infinity(); if (ok()) complain("plan: infinite level"); a = good;
    if (events_launch_ok(a, 0, 8, 4, 1, 10, 1, 2) || events_launch_ok(a, 9, 8, 4, 1, 10, 1, 2) || events_launch_ok(a, 1, 9, 4, 1, 10, 1, 2) ||
        events_launch_ok(a, 1, 8, 0, 1, 10, 1, 2) || events_launch_ok(a, 1, 8, 4, 1, 10, 1, 11) || events_launch_ok(a, 1, 8, 4, 1, 10, 1, 0) ||
        events_launch_ok(a, 1, 8, 4, uint64_t(1) << 53, 1, 1, 1))
        complain("plan: events_launch_ok accepts a bad launch");
}

// ---- reads over the fixture's ring ----------------------------------------------------------------------------------------
int column_of(uint64_t id) {
    for (int k = 0; k < 4; k++)
        if (id == sixdof_component_id(kNames[k])) return k;
    return -1;
}
sixdof_event_trigger trigger(const char* name, uint32_t element, uint32_t group, uint32_t op, uint32_t mode, double level) {
    sixdof_event_trigger t{};
    t.component_id = sixdof_component_id(name), t.element = element, t.group = group, t.op = op, t.mode = mode, t.level = level;
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
Result plain_loop(const Recorded<T>& r, const std::vector<sixdof_event_trigger>& trig, const std::vector<uint64_t>& cap, uint32_t period, uint64_t first,
                  uint64_t n_samples, uint64_t every) {
    Result out(trig.size(), cap, r.n, period, kNaN);
    const uint64_t runs = r.n / period;
    for (size_t t = 0; t < trig.size(); t++) {
        const int k = column_of(trig[t].component_id);
        for (uint64_t run = 0; run < runs; run++) {
            Walker w{trig[t].mode};
            for (uint64_t j = 0; j < n_samples; j++) {
                const uint64_t tick = first + j * every;
                const T x = r.truth[k][tick - 1][(run * period + trig[t].group) * kWidths[k] + trig[t].element];
                w.sample(tick, double(x), std::isfinite(x), compare(double(x), trig[t].op, trig[t].level));
            }
            const double planes[kPlanes] = {double(w.f.tick), w.f.value, double(w.f.before), w.f.value_before};
            for (size_t p = 0; p < kPlanes; p++) out.events[(t * kPlanes + p) * runs + run] = planes[p];
            for (size_t c = 0; c < cap.size(); c++) {
                const int ck = column_of(cap[c]);
                const uint64_t rw = period * kWidths[ck], total = r.n * kWidths[ck];
                for (uint64_t i = run * rw; i < (run + 1) * rw; i++) out.captures[c][t * total + i] = w.f.tick ? double(r.truth[ck][w.f.tick - 1][i]) : kNaN;
            }
        }
    }
    return out;
}

// samples [0, n_samples) of the range in calls that begin at the sample indices `cuts` (cuts[0] = 0): the calls before the last
// hold, the second and later ones continue
template <class T>
bool read_cut(const Recorded<T>& r, const std::vector<sixdof_event_trigger>& trig, const std::vector<uint64_t>& cap, uint32_t period, Result& out, uint64_t first,
              uint64_t n_samples, uint64_t every, const std::vector<uint64_t>& cuts, uint32_t last_flags = 0) {
    for (size_t c = 0; c < cuts.size(); c++) {
        const uint64_t lo = cuts[c], hi = c + 1 < cuts.size() ? cuts[c + 1] : n_samples;
        const bool last = c + 1 == cuts.size();
        const uint32_t flags = (c ? kContinue : 0u) | (last ? last_flags : kHold);
        if (sixdof_history_events(r.h, trig.data(), trig.size(), cap.data(), cap.size(), period, first + lo * every, hi - lo, every, last ? out.events.data() : nullptr,
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
    const double pos0 = sizeof(T) == 4 ? 640.0 : 6.4e6;
    const std::vector<sixdof_event_trigger> trig = {
        trigger("world_vel", 5, 0, SIXDOF_EVENT_LE, kCrossing, -2.0),             // crafted: small integers, NaN rows, +-inf
        trigger("world_vel", 1, period - 1, SIXDOF_EVENT_GT, kLevel, 0.0),
        trigger("world_pos", 0, 0, SIXDOF_EVENT_GE, kCrossing, pos0 + 0.5),
        trigger("force", 4, period / 2, SIXDOF_EVENT_LT, kLevel, -0.3),           // with holes: NaN in every row at every tick
        trigger("world_vel", 4, 0, SIXDOF_EVENT_LE, kCrossing, 0.0),              // crafted: +-0, denormals, the largest values
        trigger("world_accel", 3, period - 1, SIXDOF_EVENT_LT, kCrossing, 0.0),
        trigger("world_vel", 1, 0, SIXDOF_EVENT_GT, kCrossing, 0.0),              // the LEVEL trigger above, as a crossing
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
    if (n_samples >= 2) cuttings.push_back({0, n_samples / 2});
    if (n_samples >= 3) cuttings.push_back({0, n_samples / 3, 2 * n_samples / 3});
    uint64_t crossing_cut = 0;   // the sample index of the earliest crossing that has a "before" sample in the range
    for (size_t t = 0; t < trig.size() && n_samples >= 2; t++)
        for (uint64_t run = 0; run < runs; run++) {
            const double tick = want.events[(t * kPlanes) * runs + run], before = want.events[(t * kPlanes + 2) * runs + run];
            if (before != 0 && (crossing_cut == 0 || (uint64_t(tick) - first) / every < crossing_cut)) crossing_cut = (uint64_t(tick) - first) / every;
        }
    if (crossing_cut) cuttings.push_back({0, crossing_cut});
    else if (n_samples >= 8) complain(what + ": no crossing to cut at");
    for (const auto& cuts : cuttings) {
        Result cut(trig.size(), cap, n, period, -9.0);
        if (!read_cut(r, trig, cap, period, cut, first, n_samples, every, cuts, cuts.size() == 3 ? SIXDOF_EVENTS_ASYNC : 0u) || sixdof_download_wait(r.h) != SIXDOF_OK)
            return complain(what + ": in " + std::to_string(cuts.size()) + " calls: " + sixdof_last_error(r.h));
        if (!cut.same(whole)) complain(what + ": the range in " + std::to_string(cuts.size()) + " calls (second from sample " + std::to_string(cuts[1]) + ") differs from one call");
    }
    for (uint64_t segments : {uint64_t(1), uint64_t(2), uint64_t(3), n_samples, n_samples + 5}) {
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
    // events only: no captures
    Result bare(trig.size(), {}, n, period, -9.0);
    if (!read_cut(r, trig, {}, period, bare, first, n_samples, every, {0}) || !same_bits(bare.events, whole.events)) complain(what + ": n_captures = 0 differs");
    if (sixdof_sync(r.h) != SIXDOF_OK) complain(what + ": sync");
}

// Every refusal leaves the buffers and the accumulator untouched: an accumulator over ticks 5 .. 6 is made first, and continued
// over 7 .. 10 after the refusals; the result equals one call over 5 .. 10.
void refusals() {
    Recorded<double> r(24, 6, 10);   // recording since tick 3, the ring keeps 5 .. 10
    const uint64_t pos = sixdof_component_id("world_pos"), vel = sixdof_component_id("world_vel"), inertia = sixdof_component_id("inertia");
    const sixdof_event_trigger good = trigger("world_vel", 2, 1, SIXDOF_EVENT_GT, kCrossing, 0.25);
    const uint32_t period = 2;
    const size_t n_ev = kPlanes * 12, n_cap = 24 * 7;
    std::vector<double> ev(n_ev, 123.0), cap(n_cap, 123.0), want_ev(n_ev, -1.0), want_cap(n_cap, -1.0);
    double* dst[1] = {cap.data()};
    double* wdst[1] = {want_cap.data()};
    double* null_dst[1] = {nullptr};
    auto read = [&](const sixdof_event_trigger* t, size_t nt, const uint64_t* ids, size_t nc, uint32_t p, uint64_t first, uint64_t samples, uint64_t every, double* e,
                    double* const* d, uint32_t flags) { return sixdof_history_events(r.h, t, nt, ids, nc, p, first, samples, every, e, d, flags); };
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
    auto with = [&](auto change) { sixdof_event_trigger t = good; change(t); return t; };
    auto one = [&](const sixdof_event_trigger& t, uint32_t flags = 0) { return read(&t, 1, &pos, 1, period, 7, 2, 1, ev.data(), dst, flags); };
    const int bad = SIXDOF_ERR_INVALID_ARGUMENT;
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
    expect("no triggers", read(&good, 0, &pos, 1, period, 7, 2, 1, ev.data(), dst, 0), bad);
    {
        std::vector<sixdof_event_trigger> nine(9, good);
        expect("9 triggers", read(nine.data(), 9, &pos, 1, period, 7, 2, 1, ev.data(), dst, 0), bad);
    }
    expect("period = 0", read(&good, 1, &pos, 1, 0, 7, 2, 1, ev.data(), dst, 0), bad);
    expect("period does not divide n", read(&good, 1, &pos, 1, 7, 7, 2, 1, ev.data(), dst, 0), bad);
    expect("group = period", one(with([](sixdof_event_trigger& t) { t.group = 2; })), bad);
    expect("element = width", one(with([](sixdof_event_trigger& t) { t.element = 6; })), bad);
    expect("unknown op", one(with([](sixdof_event_trigger& t) { t.op = 4; })), bad);
    expect("unknown mode", one(with([](sixdof_event_trigger& t) { t.mode = 2; })), bad);
    expect("NaN level", one(with([](sixdof_event_trigger& t) { t.level = kNaN; })), bad);
    expect("infinite level", one(with([](sixdof_event_trigger& t) { t.level = -std::numeric_limits<double>::infinity(); })), bad);
    expect("trigger on inertia, which is not recorded", one(with([&](sixdof_event_trigger& t) { t.component_id = inertia; })), SIXDOF_ERR_COMPONENT_NOT_FOUND);
    expect("capture of inertia", read(&good, 1, &inertia, 1, period, 7, 2, 1, ev.data(), dst, 0), SIXDOF_ERR_COMPONENT_NOT_FOUND);
    expect("capture of inertia, held", read(&good, 1, &inertia, 1, period, 7, 2, 1, nullptr, nullptr, kHold), SIXDOF_ERR_COMPONENT_NOT_FOUND);
    expect("continue with another capture list", read(&good, 1, &vel, 1, period, 7, 4, 1, ev.data(), dst, kContinue), bad);
    expect("continue from a tick already accumulated", read(&good, 1, &pos, 1, period, 6, 5, 1, ev.data(), dst, kContinue), bad);
    expect("no samples", read(&good, 1, &pos, 1, period, 99, 0, 7, ev.data(), dst, 0), SIXDOF_OK);
    expect("no samples, continuing", read(&good, 1, &pos, 1, period, 99, 0, 7, ev.data(), dst, kContinue), SIXDOF_OK);
    if (read(&good, 1, &pos, 1, period, 7, 4, 1, ev.data(), dst, kContinue) != SIXDOF_OK) complain(std::string("refusals: continue after them: ") + sixdof_last_error(r.h));
    if (!same_bits(ev, want_ev) || !same_bits(cap, want_cap)) complain("refusals: the accumulator is not what the held call left");
    std::fill(ev.begin(), ev.end(), 123.0), std::fill(cap.begin(), cap.end(), 123.0);
    // ticks a double cannot hold: 2^53 - 2 and 2^53 - 1 are served, 2^53 is not
    const uint64_t top = uint64_t(1) << 53;
    const sixdof_event_trigger always = trigger("world_vel", 2, 1, SIXDOF_EVENT_GT, kLevel, -1e300);
    if (sixdof_set_tick(r.h, top - 3) != SIXDOF_OK || sixdof_step(r.h, 3, nullptr) != SIXDOF_OK) complain(std::string("refusals: stepping to 2^53: ") + sixdof_last_error(r.h));
    expect("a sampled tick of 2^53", read(&always, 1, &pos, 1, period, top - 2, 3, 1, ev.data(), dst, 0), bad);
    if (read(&always, 1, &pos, 1, period, top - 2, 2, 1, ev.data(), dst, 0) != SIXDOF_OK || ev[0] != double(top - 2)) complain("refusals: ticks 2^53 - 2 and 2^53 - 1 are not served");
    std::fill(ev.begin(), ev.end(), 123.0), std::fill(cap.begin(), cap.end(), 123.0);
    if (sixdof_set_history(r.h, 0) != SIXDOF_OK) complain("refusal: set_history(0)");
    expect("no ring", one(good), bad);
    expect("no ring, continuing", one(good, kContinue), bad);
}

// When SIXDOF_EVENTS_CONTINUE is refused and when it is accepted.
void continue_conditions() {
    Recorded<double> r(24, 8, 10);   // the ring keeps 3 .. 10
    const std::vector<sixdof_event_trigger> trig = {trigger("world_vel", 0, 0, SIXDOF_EVENT_GT, kCrossing, 0.5), trigger("force", 3, 2, SIXDOF_EVENT_LT, kLevel, -1.0)};
    const std::vector<uint64_t> cap = {sixdof_component_id("world_vel"), sixdof_component_id("force")}, swapped = {cap[1], cap[0]};
    const uint32_t period = 3;
    Result out(2, cap, 24, period), want(2, cap, 24, period, -9.0);
    auto call = [&](const std::vector<sixdof_event_trigger>& t, const std::vector<uint64_t>& c, uint32_t p, uint64_t first, uint64_t samples, uint64_t every, Result* to,
                    uint32_t flags) {
        return sixdof_history_events(r.h, t.data(), t.size(), c.data(), c.size(), p, first, samples, every, to ? to->events.data() : nullptr, to ? to->dst.data() : nullptr, flags);
    };
    auto refused = [&](const char* what, int rc) {
        if (rc != SIXDOF_ERR_INVALID_ARGUMENT || !*sixdof_last_error(r.h)) complain(std::string("continue ") + what + ": status " + std::to_string(rc));
        else std::printf("refusal: continue %s: %s\n", what, sixdof_last_error(r.h));
        if (out.events[0] != -7.0 || out.captures[1].back() != -7.0) complain(std::string("continue ") + what + ": something was copied");
    };
    auto changed = [&](auto change) { std::vector<sixdof_event_trigger> t = trig; change(t[1]); return t; };
    refused("with no accumulator", call(trig, cap, period, 3, 2, 1, &out, kContinue));
    if (call(trig, cap, period, 3, 2, 1, nullptr, kHold) != SIXDOF_OK) return complain(std::string("continue: hold: ") + sixdof_last_error(r.h));
    refused("with the capture list in another order", call(trig, swapped, period, 5, 2, 1, &out, kContinue));
    refused("with a shorter capture list", call(trig, {cap[0]}, period, 5, 2, 1, &out, kContinue));
    refused("with fewer triggers", call({trig[0]}, cap, period, 5, 2, 1, &out, kContinue));
    refused("with another component", call(changed([](sixdof_event_trigger& t) { t.component_id = sixdof_component_id("world_accel"); }), cap, period, 5, 2, 1, &out, kContinue));
    refused("with another element", call(changed([](sixdof_event_trigger& t) { t.element = 4; }), cap, period, 5, 2, 1, &out, kContinue));
    refused("with another group", call(changed([](sixdof_event_trigger& t) { t.group = 1; }), cap, period, 5, 2, 1, &out, kContinue));
    refused("with another op", call(changed([](sixdof_event_trigger& t) { t.op = SIXDOF_EVENT_LE; }), cap, period, 5, 2, 1, &out, kContinue));
    refused("with another mode", call(changed([](sixdof_event_trigger& t) { t.mode = kCrossing; }), cap, period, 5, 2, 1, &out, kContinue));
    refused("with another level", call(changed([](sixdof_event_trigger& t) { t.level = -1.5; }), cap, period, 5, 2, 1, &out, kContinue));
    refused("with another period", call(trig, cap, 6, 5, 2, 1, &out, kContinue));
    refused("from the last accumulated tick", call(trig, cap, period, 4, 2, 1, &out, kContinue));
    // accepted after a held call, with a gap (every = 2 from tick 6): samples 3 4 6 8 10 — the plain loop over exactly those
    if (call(trig, cap, period, 6, 3, 2, &out, kContinue) != SIXDOF_OK) return complain(std::string("continue after hold: ") + sixdof_last_error(r.h));
    {
        const uint64_t runs = 24 / period, ticks[5] = {3, 4, 6, 8, 10};
        for (size_t t = 0; t < 2; t++)
            for (uint64_t run = 0; run < runs; run++) {
                const int k = column_of(trig[t].component_id);
                Walker w{trig[t].mode};
                for (uint64_t tick : ticks) {
                    const double x = r.truth[k][tick - 1][(run * period + trig[t].group) * 6 + trig[t].element];
                    w.sample(tick, x, std::isfinite(x), compare(x, trig[t].op, trig[t].level));
                }
                const double planes[kPlanes] = {double(w.f.tick), w.f.value, double(w.f.before), w.f.value_before};
                for (size_t p = 0; p < kPlanes; p++)
                    if (std::memcmp(&planes[p], &out.events[(t * kPlanes + p) * runs + run], 8) != 0) return complain("continue after hold: plane " + std::to_string(p) + " differs");
                for (size_t c = 0; c < 2; c++)
                    for (uint64_t i = run * period * 6; i < (run + 1) * period * 6; i++) {
                        const double v = w.f.tick ? r.truth[column_of(cap[c])][w.f.tick - 1][i] : kNaN;
                        if (std::memcmp(&v, &out.captures[c][t * 24 * 6 + i], 8) != 0) return complain("continue after hold: a capture differs");
                    }
            }
    }
    auto refill = [&] {
        std::fill(out.events.begin(), out.events.end(), -7.0);
        for (auto& c : out.captures) std::fill(c.begin(), c.end(), -7.0);
    };
    refill();
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
    // after sixdof_set_history: the ring, and the accumulator with it, are new
    if (call(trig, cap, period, 3, 2, 1, nullptr, kHold) != SIXDOF_OK || sixdof_set_history(r.h, 8) != SIXDOF_OK || sixdof_step(r.h, 2, nullptr) != SIXDOF_OK)
        complain(std::string("continue: set_history: ") + sixdof_last_error(r.h));
    refused("after sixdof_set_history", call(trig, cap, period, 11, 2, 1, &out, kContinue));
    if (call(trig, cap, period, 11, 2, 1, &out, 0) != SIXDOF_OK || out.events[0] == -7.0) complain("continue: the fresh call on the new ring is wrong");
}

// More captures than one launch covers: 33 (the four Body names cycled, so every id repeats), each into its own buffer, in one
// call and in two; every buffer equals the buffer of the same name from a four-capture read.
void more_captures_than_one_launch() {
    Recorded<double> r(65, 4, 6, {true, true, false});   // the ring keeps 3 .. 6
    const std::vector<sixdof_event_trigger> trig = {trigger("world_vel", 5, 0, SIXDOF_EVENT_LE, kCrossing, -2.0), trigger("world_accel", 0, 0, SIXDOF_EVENT_GT, kLevel, 0.5)};
    std::vector<uint64_t> four_ids, many_ids;
    for (int k = 0; k < 4; k++) four_ids.push_back(sixdof_component_id(kNames[k]));
    for (int k = 0; k < 33; k++) many_ids.push_back(four_ids[k % 4]);
    Result four(2, four_ids, 65, 1);
    if (!read_cut(r, trig, four_ids, 1, four, 3, 4, 1, {0})) return complain(std::string("33 captures: ") + sixdof_last_error(r.h));
    for (uint64_t segments : {uint64_t(0), uint64_t(3)}) {
        force_segments(segments);
        Result many(2, many_ids, 65, 1);
        if (!read_cut(r, trig, many_ids, 1, many, 3, 4, 1, {0, 3})) return complain(std::string("33 captures: ") + sixdof_last_error(r.h));
        if (!same_bits(many.events, four.events)) complain("33 captures: the events differ from the four-capture read");
        for (int k = 0; k < 33; k++)
            if (!same_bits(many.captures[k], four.captures[k % 4])) complain("33 captures: buffer " + std::to_string(k) + " (" + kNames[k % 4] + ") differs from the four-capture read");
    }
    force_segments(0);
}

// What the fault sweep reads: ticks 4, 6, 8 — triggers on world_pos, a capture of force — tick 4 held, 6 and 8 continued in two
// segments, so that records, scratch, all three launches and the delivery are among the calls that fail.  dst[0] takes the event
// planes, dst[1] the capture.  After every run the ring is intact.
const std::vector<sixdof_event_trigger> kSweptTriggers = {trigger("world_pos", 0, 0, SIXDOF_EVENT_GE, kCrossing, 6.4e6 + 0.2),
                                                          trigger("world_pos", 6, 0, SIXDOF_EVENT_LT, kLevel, 6.4e6)};
const SweptRead kSwept{
    "events", {}, [](int k) { return k ? size_t(2 * 40 * 6) : size_t(2 * kPlanes * 40); },
    [](sixdof_handle* h, const uint64_t* comp, void* const dst[2], bool async) {
        const int rc = sixdof_history_events(h, kSweptTriggers.data(), 2, comp + 1, 1, 1, 4, 1, 2, nullptr, nullptr, kHold);
        double* cap[1] = {static_cast<double*>(dst[1])};
        return rc != SIXDOF_OK ? rc
                               : sixdof_history_events(h, kSweptTriggers.data(), 2, comp + 1, 1, 1, 6, 2, 2, static_cast<double*>(dst[0]), cap,
                                                       kContinue | (async ? SIXDOF_EVENTS_ASYNC : 0u));
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
    rule_exhaustive();
    values_case<double>(300, 4, 10, 27, 18, 3, crafted);     // the range wraps the ring (slots 7 .. 9, 0 .. 6), every third tick
    values_case<float>(300, 1, 10, 27, 18, 3, crafted);
    values_case<double>(300, 1, 8, 9, 3, 1, crafted);        // every recorded tick: the crafted block rotates through 7 ticks
    values_case<double>(4099, 1, 4, 5, 3, 2, random);        // a ragged last block
    values_case<float>(64, 4, 8, 8, 3, 1, random);
    values_case<double>(260, 4, 40, 42, 3, 1, random);       // 40 samples, 65 runs: one past a wavefront; the plan cuts them itself
    values_case<double>(5, 1, 40, 42, 30, 1, crafted);       // 13 samples: no multiple of the load depth nor of the segment counts
    values_case<double>(1, 1, 4, 4, 4, 1, random);           // one row, one sample
    values_case<double>(65, 1, 4, 4, 4, 1, crafted);         // one sample
    refusals();
    continue_conditions();
    more_captures_than_one_launch();
    force_segments(2);
    failure_injection("events_host_test", kSwept, {true, false, true});
    failure_injection("events_host_test", kSwept, {true, false, true}, hip_fake::kComputeFirst);
    force_segments(0);
    return verdict("events_host_test");
}
