// norms_host_test.cpp — sixdof_history_norms (sixdof_capi.cpp) over the fake runtime (hip_fake.cpp), whose launcher walks and merges
// through norms_plan.hpp — norms_value and norms_walk, the functions the kernel calls — and extremes_plan.hpp's rule in the kernels'
// time segments, under AddressSanitizer / UBSan and without FMA contraction, no GPU: `make norms_test`,
// tests/test_history_norms_host.py.
//
// The ring and the fault sweep are ring_host_fixture.hpp's.  Checked: the value function bitwise against a plain loop written
// here, count 1 to 4, with and without MINUS, f32 and f64, over +-0, denormals, values whose squares overflow, NaN and +-inf; the
// rule over every cut of random and crafted sample sequences into 2 and 3 parts, against one walk and against a plain loop; every
// plane bitwise against that plain loop over the fixture's host copy of the ring, f64 and f32, period 1 to 4, ranges that wrap the
// ring, take every k-th tick or hold one sample; one call against the same range in 2 and 3 calls (SIXDOF_NORMS_HOLD, then
// SIXDOF_NORMS_CONTINUE) and under forced segment counts; every refusal with nothing copied and the accumulator untouched; the
// conditions of SIXDOF_NORMS_CONTINUE; every fallible runtime call failed once.
#include "norms_plan.hpp"
#include "ring_host_fixture.hpp"

namespace {

constexpr size_t kPlanes = SIXDOF_NORMS_PLANES;
constexpr uint32_t kHold = SIXDOF_NORMS_HOLD, kContinue = SIXDOF_NORMS_CONTINUE, kMinus = SIXDOF_NORM_MINUS;

void force_segments(uint64_t count) { force_segments("SIXDOF_NORMS_SEGMENTS", count); }
const double kNaN = std::numeric_limits<double>::quiet_NaN();

uint64_t bits_of(double x) { uint64_t u; std::memcpy(&u, &x, 8); return u; }

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
struct Plain {
    uint64_t count = 0, tick_min = 0, tick_max = 0, first_nonfinite = 0;
    double min = kNaN, max = kNaN;
    void sample(uint64_t tick, double s) {
        if (!std::isfinite(s)) {
            if (!first_nonfinite) first_nonfinite = tick;
            return;
        }
        if (count == 0 || s < min) min = s, tick_min = tick;     // s is +0.0 or above: the IEEE compare is the order of the keys
        if (count == 0 || s > max) max = s, tick_max = tick;
        count++;
    }
    void planes(double* out, size_t stride) const {
        out[0] = double(count), out[stride] = min, out[2 * stride] = double(tick_min), out[3 * stride] = max, out[4 * stride] = double(tick_max);
        out[5 * stride] = double(first_nonfinite);
    }
};

// ---- the value ------------------------------------------------------------------------------------------------------------
template <class T, uint32_t C, bool M>
double compiled_value(const T* a, const T* b) { return sixdof::norms_value<T, C, M>(a, b); }

template <class T>
void value_function() {
    using L = std::numeric_limits<T>;
    const T big = T(std::sqrt(double(L::max())));   // its square is near the largest value of T, far below the largest double
    const std::vector<T> pool = {T(0.0), T(-0.0), L::denorm_min(), -L::denorm_min(), L::min(), T(1), T(-1), T(3), T(-4), T(0.1), T(1e-30), big, -big, L::max(), L::lowest(),
                                 L::quiet_NaN(), L::infinity(), -L::infinity(), T(6.4e6), T(6.4e6 + 1)};
    std::mt19937_64 rng(sizeof(T));
    uint64_t checked = 0, overflowed = 0;
    using Fn = double (*)(const T*, const T*);
    const Fn table[4][2] = {{compiled_value<T, 1, false>, compiled_value<T, 1, true>}, {compiled_value<T, 2, false>, compiled_value<T, 2, true>},
                            {compiled_value<T, 3, false>, compiled_value<T, 3, true>}, {compiled_value<T, 4, false>, compiled_value<T, 4, true>}};
    for (uint32_t count = 1; count <= 4; count++)
        for (int minus = 0; minus < 2; minus++) {
            // every pair of the pool in the first element (count 1: every input there is), random draws of the pool elsewhere
            for (size_t i = 0; i < pool.size(); i++)
                for (size_t j = 0; j < pool.size(); j++)
                    for (int round = 0; round < (count == 1 ? 1 : 40); round++) {
                        T a[4], b[4];
                        a[0] = pool[i], b[0] = pool[j];
                        for (uint32_t e = 1; e < 4; e++) a[e] = pool[rng() % pool.size()], b[e] = pool[rng() % pool.size()];
                        if (round % 2) for (uint32_t e = 1; e < 4; e++) a[e] = T(std::ldexp(double(rng() % 1000003), int(rng() % 40) - 20)), b[e] = T(double(rng() % 977) / 7.0);
                        const double want = plain_value(a, b, count, minus != 0), got = table[count - 1][minus](a, b);
                        const bool finite = std::isfinite(want);
                        if (finite != std::isfinite(got) || (finite && bits_of(got) != bits_of(want)))
                            return complain("value: count " + std::to_string(count) + (minus ? " minus" : "") + " differs from the plain loop");
                        if (finite && std::signbit(got)) return complain("value: a negative zero");
                        bool inputs_finite = true;
                        for (uint32_t e = 0; e < count; e++) inputs_finite = inputs_finite && std::isfinite(a[e]) && (!minus || std::isfinite(b[e]));
                        if (!inputs_finite && finite) return complain("value: a non-finite input gave a finite norm");
                        overflowed += inputs_finite && !finite;
                        checked++;
                    }
        }
    if (sizeof(T) == 8 && overflowed == 0) complain("value: no case overflowed from finite inputs");
    // f32 inputs are widened first: the square of the largest float is a finite double
    if (sizeof(T) == 4) {
        const T a[1] = {L::max()}, b[1] = {L::lowest()};
        if (!std::isfinite(sixdof::norms_value<T, 1, false>(a, b)) || !std::isfinite(sixdof::norms_value<T, 1, true>(a, b))) complain("value: f32 was not widened before the square");
    } else {
        const T a[1] = {L::max()}, b[1] = {L::lowest()}, c[2] = {T(1e154), T(1e154)};
        if (std::isfinite(sixdof::norms_value<T, 1, false>(a, b)) || std::isfinite(sixdof::norms_value<T, 1, true>(a, b)) || std::isfinite(sixdof::norms_value<T, 2, false>(c, c)))
            complain("value: an overflow from finite inputs is not non-finite");
    }
    std::printf("norms_host_test: %llu %s values agree with the plain loop\n", static_cast<unsigned long long>(checked), sizeof(T) == 4 ? "f32" : "f64");
}

// ---- the rule over every cut ---------------------------------------------------------------------------------------------
void rule_over_cuts() {
    using namespace sixdof;
    std::mt19937_64 rng(7);
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<std::vector<double>> sequences = {
        {}, {0.0}, {kNaN}, {0.0, 0.0, 0.0, 0.0}, {kNaN, inf, kNaN}, {2.0, 1.0, 1.0, 3.0, 3.0, 1.0}, {inf, 5.0, 5.0, kNaN, 5.0}, {1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0},
        {7.0, 6.0, 5.0, 4.0, 3.0, 2.0, 1.0}, {kNaN, 4.0, kNaN, 4.0, 0.0, 4.0, 0.0}, {5e-324, 0.0, 5e-324, 1.7e308, 1.7e308}};
    for (int k = 0; k < 300; k++) {
        std::vector<double> s(rng() % 13);
        for (double& x : s) {
            const uint64_t pick = rng() % 10;
            x = pick == 0 ? kNaN : pick == 1 ? inf : double(rng() % 5);      // few distinct values: ties everywhere
        }
        sequences.push_back(s);
    }
    uint64_t checked = 0;
    for (const auto& s : sequences) {
        const uint32_t len = static_cast<uint32_t>(s.size());
        auto walk = [&](uint32_t lo, uint32_t hi) {
            ExtremesRecord r = extremes_empty();
            for (uint32_t j = lo; j < hi; j++) norms_sample(r, s[j], 10 + 3 * j);
            return r;
        };
        const ExtremesRecord whole = walk(0, len);
        Plain p;
        for (uint32_t j = 0; j < len; j++) p.sample(10 + 3 * j, s[j]);
        double want[kPlanes], got[kPlanes];
        p.planes(want, 1);
        extremes_emit<double>(whole, got, 1);
        if (std::memcmp(want, got, sizeof(got)) != 0) return complain("rule: a sequence of length " + std::to_string(len) + " differs from the plain loop");
        const ExtremesRecord back = extremes_absorb<double>(got, 1);
        if (whole.count && std::memcmp(&back, &whole, sizeof(whole)) != 0) return complain("rule: absorb is not the inverse of emit");
        auto check = [&](const ExtremesRecord& merged, const char* what) {
            double planes[kPlanes];
            extremes_emit<double>(merged, planes, 1);
            if (std::memcmp(planes, want, sizeof(planes)) != 0) complain(std::string("rule: ") + what + " of a sequence of length " + std::to_string(len) + " differs from one walk");
            checked++;
        };
        for (uint32_t c1 = 0; c1 <= len; c1++) {
            check(extremes_merge(walk(0, c1), walk(c1, len)), "a cut in 2");
            for (uint32_t c2 = c1; c2 <= len; c2++) {
                check(extremes_merge(extremes_merge(walk(0, c1), walk(c1, c2)), walk(c2, len)), "a cut in 3, left first");
                check(extremes_merge(walk(0, c1), extremes_merge(walk(c1, c2), walk(c2, len))), "a cut in 3, right first");
            }
        }
    }
    std::printf("norms_host_test: %llu merges of every cut in 2 and 3 agree with one walk\n", static_cast<unsigned long long>(checked));
}

void plan_arithmetic() {
    using namespace sixdof;
    static_assert(norms_depth(1, false) == 4 && norms_depth(3, false) == 4 && norms_depth(4, false) == 4 && norms_depth(1, true) == 4 && norms_depth(2, true) == 4 &&
                      norms_depth(3, true) == 2 && norms_depth(4, true) == 2,
                  "norms_depth");
    for (uint32_t c = 1; c <= kNormsMaxCount; c++)
        for (bool m : {false, true})
            if (norms_depth(c, m) * c * (m ? 2 : 1) > kNormsMaxLoads) complain("plan: norms_depth loads more than kNormsMaxLoads");
    if (norms_segments(65536, 1024) != 1 || norms_segments(kNormsFillThreads, 1024) != 1 || norms_segments(1024, 8) != 1 || norms_segments(0, 100) != 1 ||
        norms_segments(1024, 1024) != (kNormsFillThreads + 1023) / 1024)
        complain("plan: norms_segments");
    for (uint64_t units : {uint64_t(1), uint64_t(125), uint64_t(7168), uint64_t(65535)})
        for (uint64_t ns : {uint64_t(1), uint64_t(13), uint64_t(64), uint64_t(1024), uint64_t(1) << 31}) {
            const uint32_t s = norms_segments(units, ns);
            if (s < 1 || s > ns || s > kScanMaxSegments) complain("plan: norms_segments out of range");
        }
    if (norms_scratch_index(2, 3, 1, 10, 4) != (2 * 3 + 1) * 6 * 10 + 4 || norms_out_index(2, 10, 4) != 2 * 6 * 10 + 4) complain("plan: indices");
    NormsArgs a{};
    int dummy = 0;
    a.p[0] = {&dummy, &dummy, 7, 6, 4, 3, 3, 0, 3, kNormMinus};
    auto ok = [&] { return norms_launch_ok(a, 1, 8, 4, 1, 10, 1, 2); };
    if (!ok()) complain("plan: norms_launch_ok refuses a good launch");
    const NormsArgs good = a;
    a.p[0].element_a = 5; if (ok()) complain("plan: element"); a = good;
    a.p[0].element_b = 4; if (ok()) complain("plan: minus element"); a = good;
    a.p[0].group_a = 4; if (ok()) complain("plan: group"); a = good;
    a.p[0].group_b = 4; if (ok()) complain("plan: minus group"); a = good;
    a.p[0].count = 0; if (ok()) complain("plan: count 0"); a = good;
    a.p[0].count = 5; if (ok()) complain("plan: count 5"); a = good;
    a.p[0].flags = 2; if (ok()) complain("plan: flags"); a = good;
    a.p[0].ring_b = nullptr; if (ok()) complain("plan: null ring"); a = good;
    a.p[0].flags = 0, a.p[0].ring_b = nullptr, a.p[0].element_b = 99, a.p[0].group_b = 99; if (!ok()) complain("plan: B is looked at without MINUS"); a = good;
    if (norms_launch_ok(a, 0, 8, 4, 1, 10, 1, 2) || norms_launch_ok(a, 9, 8, 4, 1, 10, 1, 2) || norms_launch_ok(a, 1, 9, 4, 1, 10, 1, 2) ||
        norms_launch_ok(a, 1, 8, 0, 1, 10, 1, 2) || norms_launch_ok(a, 1, 8, 4, 1, 10, 1, 11) || norms_launch_ok(a, 1, 8, 4, 1, 10, 1, 0) ||
        norms_launch_ok(a, 1, 8, 4, uint64_t(1) << 53, 1, 1, 1))
        complain("plan: norms_launch_ok accepts a bad launch");
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

template <class T>
std::vector<double> plain_loop(const Recorded<T>& r, const std::vector<sixdof_norm_probe>& probes, uint32_t period, const std::vector<uint64_t>& ticks) {
    const uint64_t runs = r.n / period;
    std::vector<double> out(probes.size() * kPlanes * runs, kNaN);
    for (size_t k = 0; k < probes.size(); k++) {
        const sixdof_norm_probe& p = probes[k];
        const bool minus = (p.flags & kMinus) != 0;
        const int ka = column_of(p.component_id), kb = minus ? column_of(p.minus_component_id) : ka;
        for (uint64_t run = 0; run < runs; run++) {
            Plain pl;
            for (uint64_t tick : ticks) {
                const T* a = r.truth[ka][tick - 1].data() + (run * period + p.group) * kWidths[ka] + p.element;
                const T* b = r.truth[kb][tick - 1].data() + (run * period + (minus ? p.minus_group : p.group)) * kWidths[kb] + (minus ? p.minus_element : p.element);
                pl.sample(tick, plain_value(a, b, p.count, minus));
            }
            pl.planes(out.data() + (k * kPlanes) * runs + run, runs);
        }
    }
    return out;
}
template <class T>
std::vector<double> plain_loop(const Recorded<T>& r, const std::vector<sixdof_norm_probe>& probes, uint32_t period, uint64_t first, uint64_t n_samples, uint64_t every) {
    std::vector<uint64_t> ticks;
    for (uint64_t j = 0; j < n_samples; j++) ticks.push_back(first + j * every);
    return plain_loop(r, probes, period, ticks);
}

// samples [0, n_samples) of the range in calls that begin at the sample indices `cuts` (cuts[0] = 0): the calls before the last
// hold, the second and later ones continue
template <class T>
bool read_cut(const Recorded<T>& r, const std::vector<sixdof_norm_probe>& probes, uint32_t period, std::vector<double>& out, uint64_t first, uint64_t n_samples,
              uint64_t every, const std::vector<uint64_t>& cuts, uint32_t last_flags = 0) {
    for (size_t c = 0; c < cuts.size(); c++) {
        const uint64_t lo = cuts[c], hi = c + 1 < cuts.size() ? cuts[c + 1] : n_samples;
        const bool last = c + 1 == cuts.size();
        const uint32_t flags = (c ? kContinue : 0u) | (last ? last_flags : kHold);
        if (sixdof_history_norms(r.h, probes.data(), probes.size(), period, first + lo * every, hi - lo, every, last ? out.data() : nullptr, flags) != SIXDOF_OK) return false;
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
    const std::vector<sixdof_norm_probe> probes = {
        probe("world_vel", 3, 3),                                       // |v|; crafted: +-0, denormals, the largest values (overflow), NaN rows, +-inf
        probe("world_pos", 4, 3, 0, "world_pos", 4, lastg),             // a separation of two rows of a run; period 1: a row against itself
        probe("world_pos", 4, 3, lastg, "world_accel", 0, midg),        // across components
        probe("world_pos", 0, 4, midg),                                 // the quaternion
        probe("force", 4, 1, lastg),                                    // count 1; with holes: NaN at every tick
        probe("world_vel", 1, 2, 0, "force", 2, lastg),
        probe("world_vel", 4, 1, midg),
        probe("world_accel", 0, 1, 0, "world_accel", 5, 0),             // two elements of one row
    };
    force_segments(0);
    const size_t doubles = probes.size() * kPlanes * runs;
    std::vector<double> whole(doubles, -7.0);
    if (!read_cut(r, probes, period, whole, first, n_samples, every, {0})) return complain(what + ": " + sixdof_last_error(r.h));
    const std::vector<double> want = plain_loop(r, probes, period, first, n_samples, every);
    for (size_t i = 0; i < doubles; i++)
        if (std::memcmp(&want[i], &whole[i], 8) != 0) {
            complain(what + ": probe " + std::to_string(i / (kPlanes * runs)) + " plane " + std::to_string(i / runs % kPlanes) + " run " + std::to_string(i % runs) + ": " +
                     std::to_string(whole[i]) + " != " + std::to_string(want[i]));
            break;
        }
    if (period == 1)       // ties: a row against itself is +0.0 at every tick — both ticks are the first sample, every sample counts
        for (uint64_t run = 0; run < runs; run++) {
            const double* p = whole.data() + kPlanes * runs + run;
            if (p[0] != double(n_samples) || bits_of(p[runs]) != 0 || p[2 * runs] != double(first) || bits_of(p[3 * runs]) != 0 || p[4 * runs] != double(first) || p[5 * runs] != 0)
                return complain(what + ": a row against itself is not +0.0 from the first sample on");
        }
    // cut-independence: the same range in 2 and in 3 calls, and under forced segment counts
    std::vector<std::vector<uint64_t>> cuttings;
    if (n_samples >= 2) cuttings.push_back({0, n_samples / 2}), cuttings.push_back({0, 1});
    if (n_samples >= 3) cuttings.push_back({0, n_samples / 3, 2 * n_samples / 3});
    for (const auto& cuts : cuttings) {
        std::vector<double> cut(doubles, -9.0);
        if (!read_cut(r, probes, period, cut, first, n_samples, every, cuts, cuts.size() == 3 ? SIXDOF_NORMS_ASYNC : 0u) || sixdof_download_wait(r.h) != SIXDOF_OK)
            return complain(what + ": in " + std::to_string(cuts.size()) + " calls: " + sixdof_last_error(r.h));
        if (!same_bits(cut, whole)) complain(what + ": the range in " + std::to_string(cuts.size()) + " calls (second from sample " + std::to_string(cuts[1]) + ") differs from one call");
    }
    for (uint64_t segments : {uint64_t(1), uint64_t(2), uint64_t(3), uint64_t(5), n_samples, n_samples + 5}) {
        force_segments(segments);
        std::vector<double> forced(doubles, -9.0);
        if (!read_cut(r, probes, period, forced, first, n_samples, every, {0})) return complain(what + ": " + std::to_string(segments) + " segments: " + sixdof_last_error(r.h));
        if (!same_bits(forced, whole)) complain(what + ": " + std::to_string(segments) + " forced segments differ from the plan's choice");
        for (const auto& cuts : cuttings) {     // segments and calls together: the accumulator comes first in the merge launch
            std::vector<double> both(doubles, -9.0);
            if (!read_cut(r, probes, period, both, first, n_samples, every, cuts) || !same_bits(both, whole))
                complain(what + ": " + std::to_string(segments) + " forced segments in " + std::to_string(cuts.size()) + " calls differ");
        }
    }
    force_segments(0);
    // one probe alone is its block of the eight
    for (size_t k : {size_t(0), probes.size() - 1}) {
        std::vector<double> one(kPlanes * runs, -9.0);
        if (!read_cut(r, {probes[k]}, period, one, first, n_samples, every, {0}) || std::memcmp(one.data(), whole.data() + k * kPlanes * runs, one.size() * 8) != 0)
            complain(what + ": probe " + std::to_string(k) + " alone differs");
    }
    if (sixdof_sync(r.h) != SIXDOF_OK) complain(what + ": sync");
}

// Every refusal leaves the buffer and the accumulator untouched: an accumulator over ticks 5 .. 6 is made first, and continued
// over 7 .. 10 after the refusals; the result equals one call over 5 .. 10.
void refusals() {
    Recorded<double> r(24, 6, 10);   // recording since tick 3, the ring keeps 5 .. 10
    const uint64_t inertia = sixdof_component_id("inertia");
    const sixdof_norm_probe good = probe("world_vel", 3, 3, 1, "world_pos", 4, 0);
    const uint32_t period = 2;
    const size_t doubles = kPlanes * 12;
    std::vector<double> buf(doubles, 123.0), want(doubles, -1.0);
    auto read = [&](const sixdof_norm_probe* p, size_t np, uint32_t per, uint64_t first, uint64_t samples, uint64_t every, double* dst, uint32_t flags) {
        return sixdof_history_norms(r.h, p, np, per, first, samples, every, dst, flags);
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
    auto with = [&](auto change) { sixdof_norm_probe p = good; change(p); return p; };
    auto one = [&](const sixdof_norm_probe& p, uint32_t flags = 0) { return read(&p, 1, period, 7, 2, 1, buf.data(), flags); };
    const int bad = SIXDOF_ERR_INVALID_ARGUMENT;
    expect("every = 0", read(&good, 1, period, 7, 2, 0, buf.data(), 0), bad);
    expect("fallen out of the ring", read(&good, 1, period, 4, 2, 1, buf.data(), 0), bad);
    expect("beyond tick", read(&good, 1, period, 9, 3, 1, buf.data(), 0), bad);
    expect("last sample beyond tick", read(&good, 1, period, 5, 3, 3, buf.data(), 0), bad);
    expect("unknown flags", one(good, 8u), bad);
    expect("null probes", read(nullptr, 1, period, 7, 2, 1, buf.data(), 0), bad);
    expect("null buffer", read(&good, 1, period, 7, 2, 1, nullptr, 0), bad);
    expect("null buffer, continuing", read(&good, 1, period, 7, 2, 1, nullptr, kContinue), bad);
    expect("null probes, held", read(nullptr, 1, period, 7, 2, 1, nullptr, kHold), bad);
    expect("no probes", read(&good, 0, period, 7, 2, 1, buf.data(), 0), bad);
    {
        std::vector<sixdof_norm_probe> nine(9, good);
        expect("9 probes", read(nine.data(), 9, period, 7, 2, 1, buf.data(), 0), bad);
    }
    expect("period = 0", read(&good, 1, 0, 7, 2, 1, buf.data(), 0), bad);
    expect("period does not divide n", read(&good, 1, 7, 7, 2, 1, buf.data(), 0), bad);
    expect("count = 0", one(with([](sixdof_norm_probe& p) { p.count = 0; })), bad);
    expect("count = 5", one(with([](sixdof_norm_probe& p) { p.count = 5; })), bad);
    expect("element + count above the width", one(with([](sixdof_norm_probe& p) { p.element = 4; })), bad);
    expect("minus_element + count above the width", one(with([](sixdof_norm_probe& p) { p.minus_element = 5; })), bad);
    expect("element far above the width", one(with([](sixdof_norm_probe& p) { p.element = 0xffffffffu; })), bad);
    expect("group = period", one(with([](sixdof_norm_probe& p) { p.group = 2; })), bad);
    expect("minus_group = period", one(with([](sixdof_norm_probe& p) { p.minus_group = 2; })), bad);
    expect("unknown probe flags", one(with([](sixdof_norm_probe& p) { p.flags = 3; })), bad);
    expect("a probe of inertia, which is not recorded", one(with([&](sixdof_norm_probe& p) { p.component_id = inertia; })), SIXDOF_ERR_COMPONENT_NOT_FOUND);
    expect("minus inertia", one(with([&](sixdof_norm_probe& p) { p.minus_component_id = inertia; })), SIXDOF_ERR_COMPONENT_NOT_FOUND);
    {
        const sixdof_norm_probe p = with([&](sixdof_norm_probe& q) { q.minus_component_id = inertia; });
        expect("minus inertia, held", read(&p, 1, period, 7, 2, 1, nullptr, kHold), SIXDOF_ERR_COMPONENT_NOT_FOUND);
    }
    expect("continue with another probe", one(with([](sixdof_norm_probe& p) { p.element = 2; }), kContinue), bad);
    expect("continue from a tick already accumulated", read(&good, 1, period, 6, 5, 1, buf.data(), kContinue), bad);
    expect("no samples", read(&good, 1, period, 99, 0, 7, buf.data(), 0), SIXDOF_OK);
    expect("no samples, continuing", read(&good, 1, period, 99, 0, 7, buf.data(), kContinue), SIXDOF_OK);
    if (read(&good, 1, period, 7, 4, 1, buf.data(), kContinue) != SIXDOF_OK) complain(std::string("refusals: continue after them: ") + sixdof_last_error(r.h));
    if (!same_bits(buf, want)) complain("refusals: the accumulator is not what the held call left");
    std::fill(buf.begin(), buf.end(), 123.0);
    // without MINUS the three minus_ fields are not read: whatever they hold, the probe is served
    {
        sixdof_norm_probe plain = probe("world_vel", 3, 3, 1), noisy = plain;
        noisy.minus_component_id = inertia, noisy.minus_element = 99, noisy.minus_group = 99;
        std::vector<double> a(doubles, -1.0), b(doubles, -2.0);
        if (read(&plain, 1, period, 5, 6, 1, a.data(), 0) != SIXDOF_OK || read(&noisy, 1, period, 5, 6, 1, b.data(), 0) != SIXDOF_OK || !same_bits(a, b))
            complain("refusals: the minus_ fields are read without SIXDOF_NORM_MINUS");
    }
    // ticks a double cannot hold: 2^53 - 2 and 2^53 - 1 are served, 2^53 is not
    const uint64_t top = uint64_t(1) << 53;
    if (sixdof_set_tick(r.h, top - 3) != SIXDOF_OK || sixdof_step(r.h, 3, nullptr) != SIXDOF_OK) complain(std::string("refusals: stepping to 2^53: ") + sixdof_last_error(r.h));
    expect("a sampled tick of 2^53", read(&good, 1, period, top - 2, 3, 1, buf.data(), 0), bad);
    if (read(&good, 1, period, top - 2, 2, 1, buf.data(), 0) != SIXDOF_OK || buf[2 * 12] < double(top - 2)) complain("refusals: ticks 2^53 - 2 and 2^53 - 1 are not served");
    std::fill(buf.begin(), buf.end(), 123.0);
    if (sixdof_set_history(r.h, 0) != SIXDOF_OK) complain("refusal: set_history(0)");
    expect("no ring", one(good), bad);
    expect("no ring, continuing", one(good, kContinue), bad);
}

// When SIXDOF_NORMS_CONTINUE is refused and when it is accepted.
void continue_conditions() {
    Recorded<double> r(24, 8, 10);   // the ring keeps 3 .. 10
    const std::vector<sixdof_norm_probe> probes = {probe("world_vel", 0, 3), probe("force", 3, 2, 2, "world_accel", 1, 1)};
    const uint32_t period = 3;
    const uint64_t runs = 24 / period;
    const size_t doubles = 2 * kPlanes * runs;
    std::vector<double> out(doubles, -7.0), want(doubles, -9.0);
    auto call = [&](const std::vector<sixdof_norm_probe>& p, uint32_t per, uint64_t first, uint64_t samples, uint64_t every, std::vector<double>* to, uint32_t flags) {
        return sixdof_history_norms(r.h, p.data(), p.size(), per, first, samples, every, to ? to->data() : nullptr, flags);
    };
    auto refused = [&](const char* what, int rc) {
        if (rc != SIXDOF_ERR_INVALID_ARGUMENT || !*sixdof_last_error(r.h)) complain(std::string("continue ") + what + ": status " + std::to_string(rc));
        else std::printf("refusal: continue %s: %s\n", what, sixdof_last_error(r.h));
        if (out[0] != -7.0 || out.back() != -7.0) complain(std::string("continue ") + what + ": something was copied");
    };
    auto changed = [&](auto change) { std::vector<sixdof_norm_probe> p = probes; change(p[1]); return p; };
    refused("with no accumulator", call(probes, period, 3, 2, 1, &out, kContinue));
    if (call(probes, period, 3, 2, 1, nullptr, kHold) != SIXDOF_OK) return complain(std::string("continue: hold: ") + sixdof_last_error(r.h));
    refused("with fewer probes", call({probes[0]}, period, 5, 2, 1, &out, kContinue));
    refused("with the probes in another order", call({probes[1], probes[0]}, period, 5, 2, 1, &out, kContinue));
    refused("with another component", call(changed([](sixdof_norm_probe& p) { p.component_id = sixdof_component_id("world_vel"); }), period, 5, 2, 1, &out, kContinue));
    refused("with another minus component", call(changed([](sixdof_norm_probe& p) { p.minus_component_id = sixdof_component_id("world_vel"); }), period, 5, 2, 1, &out, kContinue));
    refused("with another element", call(changed([](sixdof_norm_probe& p) { p.element = 4; }), period, 5, 2, 1, &out, kContinue));
    refused("with another minus element", call(changed([](sixdof_norm_probe& p) { p.minus_element = 0; }), period, 5, 2, 1, &out, kContinue));
    refused("with another group", call(changed([](sixdof_norm_probe& p) { p.group = 1; }), period, 5, 2, 1, &out, kContinue));
    refused("with another minus group", call(changed([](sixdof_norm_probe& p) { p.minus_group = 0; }), period, 5, 2, 1, &out, kContinue));
    refused("with another count", call(changed([](sixdof_norm_probe& p) { p.count = 1; }), period, 5, 2, 1, &out, kContinue));
    refused("with other flags", call(changed([](sixdof_norm_probe& p) { p.flags = 0; }), period, 5, 2, 1, &out, kContinue));
    refused("with another period", call(probes, 6, 5, 2, 1, &out, kContinue));
    refused("from the last accumulated tick", call(probes, period, 4, 2, 1, &out, kContinue));
    // accepted after a held call, with a gap (every = 2 from tick 6): samples 3 4 6 8 10 — the plain loop over exactly those
    if (call(probes, period, 6, 3, 2, &out, kContinue) != SIXDOF_OK) return complain(std::string("continue after hold: ") + sixdof_last_error(r.h));
    if (!same_bits(out, plain_loop(r, probes, period, {3, 4, 6, 8, 10}))) complain("continue after hold differs from the plain loop over its samples");
    std::fill(out.begin(), out.end(), -7.0);
    // a delivered call leaves an accumulator too: continue it
    if (call(probes, period, 3, 4, 1, &want, 0) != SIXDOF_OK || call(probes, period, 7, 4, 1, &want, kContinue) != SIXDOF_OK || call(probes, period, 3, 8, 1, &out, 0) != SIXDOF_OK ||
        !same_bits(out, want))
        complain("continue after a delivered call differs from one call");
    std::fill(out.begin(), out.end(), -7.0);
    // after a call that failed in the runtime: refused, and a fresh call is correct
    if (call(probes, period, 3, 2, 1, nullptr, kHold) != SIXDOF_OK) complain("continue: second hold");
    hip_fake::fail_after(0);
    const int rc = call(probes, period, 5, 2, 1, nullptr, kHold | kContinue);
    const bool fired = hip_fake::fired();
    hip_fake::fail_after(-1);
    if (rc != SIXDOF_ERR_BACKEND || !fired) complain("continue: the injected fault did not fail the call");
    refused("after a failed call", call(probes, period, 7, 2, 1, &out, kContinue));
    if (call(probes, period, 3, 8, 1, &out, 0) != SIXDOF_OK || !same_bits(out, want)) complain("continue: the fresh call after a failed one is wrong");
    std::fill(out.begin(), out.end(), -7.0);
    // the other scans keep accumulators of their own: an extremes read in between does not disturb this one
    {
        const uint64_t vel = sixdof_component_id("world_vel");
        std::vector<double> ext(kPlanes * 24 * 6);
        double* dst[1] = {ext.data()};
        if (call(probes, period, 3, 4, 1, nullptr, kHold) != SIXDOF_OK || sixdof_history_extremes(r.h, &vel, 1, 3, 8, 1, dst, 0) != SIXDOF_OK ||
            call(probes, period, 7, 4, 1, &out, kContinue) != SIXDOF_OK || !same_bits(out, want))
            complain("continue: another scan in between disturbs the accumulator");
        std::fill(out.begin(), out.end(), -7.0);
    }
    // after sixdof_set_history: the ring, and the accumulator with it, are new
    if (call(probes, period, 3, 2, 1, nullptr, kHold) != SIXDOF_OK || sixdof_set_history(r.h, 8) != SIXDOF_OK || sixdof_step(r.h, 2, nullptr) != SIXDOF_OK)
        complain(std::string("continue: set_history: ") + sixdof_last_error(r.h));
    refused("after sixdof_set_history", call(probes, period, 11, 2, 1, &out, kContinue));
    if (call(probes, period, 11, 2, 1, &out, 0) != SIXDOF_OK || out[0] == -7.0) complain("continue: the fresh call on the new ring is wrong");
}

// What the fault sweep reads: ticks 4, 6, 8 — |r| of world_pos, and world_pos against force, whose element 4 is NaN in every row —
// tick 4 held, 6 and 8 continued in two segments, so that scratch, both launches and the delivery are among the calls that fail.
// dst[0] takes the planes, dst[1] nothing.  After every run the ring is intact.
const std::vector<sixdof_norm_probe> kSweptProbes = {probe("world_pos", 4, 3), probe("world_pos", 4, 3, 0, "force", 2, 0), probe("world_pos", 0, 4, 0, "force", 0, 0)};
const SweptRead kSwept{
    "norms", {}, [](int k) { return k ? size_t(1) : size_t(3 * kPlanes * 40); },
    [](sixdof_handle* h, const uint64_t*, void* const dst[2], bool async) {
        const int rc = sixdof_history_norms(h, kSweptProbes.data(), 3, 1, 4, 1, 2, nullptr, kHold);
        return rc != SIXDOF_OK ? rc : sixdof_history_norms(h, kSweptProbes.data(), 3, 1, 6, 2, 2, static_cast<double*>(dst[0]), kContinue | (async ? SIXDOF_NORMS_ASYNC : 0u));
    },
    [](const Recorded<double>& r, bool fault_free, const std::vector<double> want[2], const std::string& run) {
        if (fault_free) {
            const std::vector<double> plain = plain_loop(r, kSweptProbes, 1, 4, 3, 2);
            if (!same_bits(want[0], plain)) complain(run + ": the values are not the plain loop's");
            if (plain[0] != 3.0 || plain[kPlanes * 40] != 0.0 || plain[(kPlanes + 5) * 40] != 4.0) complain(run + ": the swept read does not see what it was made to see");
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
    values_case<double>(2, 2, 4, 4, 4, 1, random);           // one run, one sample
    values_case<double>(65, 1, 4, 4, 4, 1, crafted);         // one sample
    refusals();
    continue_conditions();
    force_segments(2);
    failure_injection("norms_host_test", kSwept, {true, false, true});
    failure_injection("norms_host_test", kSwept, {true, false, true}, hip_fake::kComputeFirst);
    force_segments(0);
    return verdict("norms_host_test");
}
