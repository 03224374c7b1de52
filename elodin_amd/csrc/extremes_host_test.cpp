// extremes_host_test.cpp — sixdof_history_extremes (sixdof_capi.cpp) over the fake runtime (hip_fake.cpp), whose launcher walks and
// merges through extremes_plan.hpp in the kernels' time segments and the kernels' own loop (time_scan.hpp), under AddressSanitizer / UBSan, no GPU: `make extremes_test`,
// tests/test_history_extremes_host.py.
//
// The ring and the fault sweep are ring_host_fixture.hpp's.  Checked: every plane bitwise against a plain loop over the fixture's
// host copy of the ring, f64 and f32, over random blocks and the crafted block rotated by the tick (ties at several ticks, +-0,
// denormals, +-inf, NaN rows, a NaN that comes and goes, an element that is NaN at every tick); ranges that wrap the ring, take
// every k-th tick or hold one sample; one call against the same range in 2 and 3 calls (SIXDOF_EXTREMES_HOLD, then
// SIXDOF_EXTREMES_CONTINUE) and against forced segment counts; every refusal with nothing copied and the accumulator untouched;
// the conditions of SIXDOF_EXTREMES_CONTINUE; 33 component entries; every fallible runtime call failed once.
#include "extremes_plan.hpp"
#include "ring_host_fixture.hpp"

namespace {

using sixdof::QuantileBits;
constexpr size_t kPlanes = SIXDOF_EXTREMES_PLANES;
constexpr uint32_t kHold = SIXDOF_EXTREMES_HOLD, kContinue = SIXDOF_EXTREMES_CONTINUE;

void force_segments(uint64_t count) { force_segments("SIXDOF_EXTREMES_SEGMENTS", count); }

// The six planes [6][n * w] of column k over the samples first, first + every, ...: a plain loop over what was uploaded.
template <class T>
std::vector<double> plain_loop(const Recorded<T>& r, int k, uint64_t first, uint64_t n_samples, uint64_t every) {
    using B = QuantileBits<T>;
    const uint64_t total = r.n * kWidths[k];
    std::vector<double> out(kPlanes * total);
    for (uint64_t i = 0; i < total; i++) {
        uint64_t count = 0, key_min = 0, key_max = 0, tick_min = 0, tick_max = 0, first_nonfinite = 0;
        T min = std::numeric_limits<T>::quiet_NaN(), max = min;
        for (uint64_t j = 0; j < n_samples; j++) {
            const uint64_t tick = first + j * every;
            const T x = r.truth[k][tick - 1][i];
            if (!std::isfinite(x)) {
                if (!first_nonfinite) first_nonfinite = tick;
                continue;
            }
            const uint64_t key = B::key(B::raw(x));
            if (count == 0 || key < key_min) key_min = key, min = x, tick_min = tick;
            if (count == 0 || key > key_max) key_max = key, max = x, tick_max = tick;
            count++;
        }
        const double planes[kPlanes] = {double(count), double(min), double(tick_min), double(max), double(tick_max), double(first_nonfinite)};
        for (size_t p = 0; p < kPlanes; p++) out[p * total + i] = planes[p];
    }
    return out;
}

// The four Body columns of one handle, read in one call or in several.
struct FourColumns {
    uint64_t comp[4];
    std::vector<double> out[4];
    double* dst[4];
    explicit FourColumns(uint64_t n, double fill = -7.0) {
        for (int k = 0; k < 4; k++) comp[k] = sixdof_component_id(kNames[k]), out[k].assign(kPlanes * n * kWidths[k], fill), dst[k] = out[k].data();
    }
    bool same(const FourColumns& o) const {
        for (int k = 0; k < 4; k++)
            if (!same_bits(out[k], o.out[k])) return false;
        return true;
    }
};
// samples [0, n_samples) of the range in `calls` calls: the calls before the last hold, the second and later ones continue
template <class T>
bool read_in_calls(const Recorded<T>& r, FourColumns& f, uint64_t first, uint64_t n_samples, uint64_t every, uint64_t calls, uint32_t last_flags = 0) {
    for (uint64_t c = 0; c < calls; c++) {
        const uint64_t lo = n_samples * c / calls, hi = n_samples * (c + 1) / calls;
        const uint32_t flags = (c ? kContinue : 0u) | (c + 1 < calls ? kHold : last_flags);
        if (sixdof_history_extremes(r.h, f.comp, 4, first + lo * every, hi - lo, every, c + 1 < calls ? nullptr : f.dst, flags) != SIXDOF_OK) return false;
    }
    return true;
}

template <class T>
void values_case(uint64_t n, uint64_t ring, uint64_t ticks, uint64_t first, uint64_t every, RecordOptions o) {
    Recorded<T> r(n, ring, ticks, o);
    const uint64_t n_samples = (ticks - first) / every + 1;
    const std::string what = std::string(sizeof(T) == 4 ? "f32" : "f64") + " n " + std::to_string(n) + " samples " + std::to_string(n_samples) + (o.crafted_vel ? " crafted" : "");
    force_segments(0);
    FourColumns whole(n);
    if (!read_in_calls(r, whole, first, n_samples, every, 1)) return complain(what + ": " + sixdof_last_error(r.h));
    for (int k = 0; k < 4; k++) {
        const std::vector<double> want = plain_loop(r, k, first, n_samples, every);
        if (same_bits(whole.out[k], want)) continue;
        for (size_t i = 0; i < want.size(); i++)
            if (std::memcmp(&want[i], &whole.out[k][i], 8) != 0) {
                const uint64_t total = n * kWidths[k];
                complain(what + ": " + kNames[k] + " plane " + std::to_string(i / total) + " element " + std::to_string(i % total) + ": " + std::to_string(whole.out[k][i]) +
                         " != " + std::to_string(want[i]));
                break;
            }
    }
    // cut-independence: the same range in 2 and in 3 calls, and under forced segment counts
    for (uint64_t calls : {uint64_t(2), uint64_t(3)}) {
        if (calls > n_samples) continue;
        FourColumns cut(n, -9.0);
        if (!read_in_calls(r, cut, first, n_samples, every, calls, calls == 3 ? SIXDOF_EXTREMES_ASYNC : 0u) || sixdof_download_wait(r.h) != SIXDOF_OK)
            return complain(what + ": in " + std::to_string(calls) + " calls: " + sixdof_last_error(r.h));
        if (!cut.same(whole)) complain(what + ": the range in " + std::to_string(calls) + " calls differs from one call");
    }
    for (uint64_t segments : {uint64_t(1), uint64_t(2), uint64_t(3), n_samples, n_samples + 5}) {
        force_segments(segments);
        FourColumns forced(n, -9.0);
        if (!read_in_calls(r, forced, first, n_samples, every, 1)) return complain(what + ": " + std::to_string(segments) + " segments: " + sixdof_last_error(r.h));
        if (!forced.same(whole)) complain(what + ": " + std::to_string(segments) + " forced segments differ from the plan's choice");
        if (n_samples >= 2) {     // segments and calls together: the accumulator comes first in the merge launch
            FourColumns both(n, -9.0);
            if (!read_in_calls(r, both, first, n_samples, every, 2) || !both.same(whole)) complain(what + ": " + std::to_string(segments) + " forced segments in 2 calls differ");
        }
    }
    force_segments(0);
    if (sixdof_sync(r.h) != SIXDOF_OK) complain(what + ": sync");
}

// The plan's own cut, and its limits.
void plan_arithmetic() {
    using namespace sixdof;
    if (extremes_segments(65536 * 7, 1024) != 1 || extremes_segments(1024 * 7, 1024) < 2 || extremes_segments(1024 * 7, 8) != 1 || extremes_segments(0, 100) != 1)
        complain("plan: extremes_segments");
    for (uint64_t total : {uint64_t(1), uint64_t(125), uint64_t(7168), uint64_t(65535)})
        for (uint64_t ns : {uint64_t(1), uint64_t(13), uint64_t(64), uint64_t(1024), uint64_t(1) << 31}) {
            const uint32_t s = extremes_segments(total, ns);
            if (s < 1 || s > ns || s > kScanMaxSegments) complain("plan: extremes_segments out of range");
            uint64_t covered = 0;
            for (uint32_t g = 0; g < s; g++) {
                const uint64_t lo = scan_segment_start(ns, s, g), hi = scan_segment_start(ns, s, g + 1);
                if (hi <= lo || lo != covered) complain("plan: the segments do not tile the samples");
                covered = hi;
            }
            if (covered != ns) complain("plan: the segments do not end on the last sample");
        }
    if (scan_clamp_segments(9, 4) != 4 || scan_clamp_segments(1u << 20, 1u << 24) != kScanMaxSegments) complain("plan: scan_clamp_segments");
    if (scan_fit_segments(8, 1000, kExtremesFields, 48 * 1000 * 3) != 3 || scan_fit_segments(8, 1000, kExtremesFields, 48 * 1000) != 1 || scan_fit_segments(1, 1u << 30, kExtremesFields, 1) != 1) complain("plan: scan_fit_segments");
    if (scan_scratch_bytes(1, 1000, kExtremesFields) != 0 || scan_scratch_bytes(3, 1000, kExtremesFields) != 3 * 48 * 1000) complain("plan: scan_scratch_bytes");
    const uint64_t top = uint64_t(1) << 53;
    if (!scan_ticks_ok(top - 1, 1, 1) || scan_ticks_ok(top - 1, 2, 1) || scan_ticks_ok(top, 1, 1) || !scan_ticks_ok(1, 3, (top - 2) / 2) ||
        scan_ticks_ok(2, 3, (top - 2) / 2) || scan_ticks_ok(1, 2, ~uint64_t(0)) || scan_ticks_ok(0, 1, 1))
        complain("plan: scan_ticks_ok");
    // the slot a walking thread advances by an add and a compare is the slot of the next sample
    for (uint64_t ring : {uint64_t(1), uint64_t(5), uint64_t(8), uint64_t(1) << 32})
        for (uint64_t every : {uint64_t(1), uint64_t(3), uint64_t(8), uint64_t(13), (uint64_t(1) << 32) + 3})
            for (uint64_t first : {uint64_t(1), uint64_t(7), uint64_t(1) << 40}) {
                uint64_t slot = sample_slot(first, 0, every, ring);
                for (uint64_t j = 1; j < 20; j++) {
                    slot = next_sample_slot(slot, every % ring, ring);
                    if (slot != sample_slot(first, j, every, ring)) complain("plan: next_sample_slot leaves the range's slots");
                }
            }
    // the rule: associative in time order, ties keep the earlier tick
    ExtremesRecord a = extremes_empty(), b = extremes_empty(), all = extremes_empty();
    const uint64_t keys[6] = {50, 40, 40, 90, 90, 40};
    for (uint64_t t = 0; t < 6; t++) {
        extremes_accumulate(t < 3 ? a : b, keys[t], t + 1, t != 1);
        extremes_accumulate(all, keys[t], t + 1, t != 1);
    }
    const ExtremesRecord m = extremes_merge(a, b);
    if (std::memcmp(&m, &all, sizeof(m)) != 0 || m.count != 5 || m.tick_min != 3 || m.tick_max != 4 || m.first_nonfinite != 2) complain("plan: merge of two halves differs from one walk");
    const ExtremesRecord e = extremes_merge(extremes_empty(), extremes_merge(all, extremes_empty()));
    if (std::memcmp(&e, &all, sizeof(e)) != 0) complain("plan: the empty record is not the identity");
}

// Every refusal leaves the buffers and the accumulator untouched: an accumulator over ticks 5 .. 6 is made first, and continued
// over 7 .. 10 after the refusals; the result equals one call over 5 .. 10.
void refusals() {
    Recorded<double> r(24, 6, 10);   // recording since tick 3, the ring keeps 5 .. 10
    const uint64_t pos = sixdof_component_id("world_pos"), vel = sixdof_component_id("world_vel"), inertia = sixdof_component_id("inertia");
    std::vector<double> buf(kPlanes * 24 * 7, 123.0), want(buf.size(), -1.0);
    double* dst[1] = {buf.data()};
    double* wdst[1] = {want.data()};
    double* null_dst[1] = {nullptr};
    if (sixdof_history_extremes(r.h, &pos, 1, 5, 6, 1, wdst, 0) != SIXDOF_OK) return complain(std::string("refusals: ") + sixdof_last_error(r.h));
    if (sixdof_history_extremes(r.h, &pos, 1, 5, 2, 1, nullptr, kHold) != SIXDOF_OK) return complain(std::string("refusals: hold: ") + sixdof_last_error(r.h));
    auto expect = [&](const char* what, int rc, int status) {
        if (rc != status) complain(std::string("refusal: ") + what + ": status " + std::to_string(rc) + ", expected " + std::to_string(status));
        else if (status != SIXDOF_OK && !*sixdof_last_error(r.h)) complain(std::string("refusal: ") + what + ": no message");
        if (status != SIXDOF_OK) std::printf("refusal: %s: %s\n", what, sixdof_last_error(r.h));
        for (double v : buf)
            if (v != 123.0) return complain(std::string("refusal: ") + what + ": something was copied"), void();
    };
    auto read = [&](const uint64_t* comp, uint64_t first, uint64_t samples, uint64_t every, double* const* d, uint32_t flags) {
        return sixdof_history_extremes(r.h, comp, 1, first, samples, every, d, flags);
    };
    expect("every = 0", read(&pos, 7, 2, 0, dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("fallen out of the ring", read(&pos, 4, 2, 1, dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("beyond tick", read(&pos, 9, 3, 1, dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("last sample beyond tick", read(&pos, 5, 3, 3, dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("unknown flags", read(&pos, 7, 2, 1, dst, 8u), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("null component ids", read(nullptr, 7, 2, 1, dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("null buffer", read(&pos, 7, 2, 1, null_dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("null buffer list", read(&pos, 7, 2, 1, nullptr, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("null buffer, continuing", read(&pos, 7, 2, 1, null_dst, kContinue), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("inertia is not recorded", read(&inertia, 7, 2, 1, dst, 0), SIXDOF_ERR_COMPONENT_NOT_FOUND);
    expect("inertia is not recorded, held", read(&inertia, 7, 2, 1, nullptr, kHold), SIXDOF_ERR_COMPONENT_NOT_FOUND);
    expect("continue with another component list", read(&vel, 7, 4, 1, dst, kContinue), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("continue from a tick already accumulated", read(&pos, 6, 5, 1, dst, kContinue), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("no samples", read(&pos, 99, 0, 7, dst, 0), SIXDOF_OK);
    expect("no samples, continuing", read(&pos, 99, 0, 7, dst, kContinue), SIXDOF_OK);
    if (read(&pos, 7, 4, 1, dst, kContinue) != SIXDOF_OK) complain(std::string("refusals: continue after them: ") + sixdof_last_error(r.h));
    if (!same_bits(buf, want)) complain("refusals: the accumulator is not what the held call left");
    std::fill(buf.begin(), buf.end(), 123.0);
    // ticks a double cannot hold: 2^53 - 2 and 2^53 - 1 are served, 2^53 is not
    const uint64_t top = uint64_t(1) << 53;
    if (sixdof_set_tick(r.h, top - 3) != SIXDOF_OK || sixdof_step(r.h, 3, nullptr) != SIXDOF_OK) complain(std::string("refusals: stepping to 2^53: ") + sixdof_last_error(r.h));
    expect("a sampled tick of 2^53", read(&pos, top - 2, 3, 1, dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    if (read(&pos, top - 2, 2, 1, dst, 0) != SIXDOF_OK || buf[2 * 24 * 7] != double(top - 2)) complain("refusals: ticks 2^53 - 2 and 2^53 - 1 are not served");
    std::fill(buf.begin(), buf.end(), 123.0);
    if (sixdof_set_history(r.h, 0) != SIXDOF_OK) complain("refusal: set_history(0)");
    expect("no ring", read(&pos, 7, 2, 1, dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("no ring, continuing", read(&pos, 7, 2, 1, dst, kContinue), SIXDOF_ERR_INVALID_ARGUMENT);
}

// When SIXDOF_EXTREMES_CONTINUE is refused and when it is accepted.
void continue_conditions() {
    Recorded<double> r(24, 8, 10);   // the ring keeps 3 .. 10
    const uint64_t comp[2] = {sixdof_component_id("world_vel"), sixdof_component_id("force")}, swapped[2] = {comp[1], comp[0]};
    std::vector<double> out[2], want[2];
    double *dst[2], *wdst[2];
    for (int k = 0; k < 2; k++) out[k].assign(kPlanes * 24 * 6, -7.0), want[k].assign(kPlanes * 24 * 6, -9.0), dst[k] = out[k].data(), wdst[k] = want[k].data();
    auto refused = [&](const char* what, int rc) {
        if (rc != SIXDOF_ERR_INVALID_ARGUMENT || !*sixdof_last_error(r.h)) complain(std::string("continue ") + what + ": status " + std::to_string(rc));
        else std::printf("refusal: continue %s: %s\n", what, sixdof_last_error(r.h));
        if (out[0][0] != -7.0 || out[1].back() != -7.0) complain(std::string("continue ") + what + ": something was copied");
    };
    refused("with no accumulator", sixdof_history_extremes(r.h, comp, 2, 3, 2, 1, dst, kContinue));
    if (sixdof_history_extremes(r.h, comp, 2, 3, 2, 1, nullptr, kHold) != SIXDOF_OK) return complain(std::string("continue: hold: ") + sixdof_last_error(r.h));
    refused("with the component list in another order", sixdof_history_extremes(r.h, swapped, 2, 5, 2, 1, dst, kContinue));
    refused("with a shorter component list", sixdof_history_extremes(r.h, comp, 1, 5, 2, 1, dst, kContinue));
    refused("from the last accumulated tick", sixdof_history_extremes(r.h, comp, 2, 4, 2, 1, dst, kContinue));
    // accepted after a held call, with a gap (every = 2 from tick 6): samples 3 4 6 8 10
    if (sixdof_history_extremes(r.h, comp, 2, 6, 3, 2, dst, kContinue) != SIXDOF_OK) return complain(std::string("continue after hold: ") + sixdof_last_error(r.h));
    for (int k = 0; k < 2; k++) {
        // the plain loop over 3 4 and over 6 8 10, merged by the rule's own words: count adds, strictly smaller / larger replaces
        const std::vector<double> a = plain_loop(r, k ? 3 : 1, 3, 2, 1), b = plain_loop(r, k ? 3 : 1, 6, 3, 2);
        const uint64_t total = 24 * 6;
        for (uint64_t i = 0; i < total; i++) {
            using B = QuantileBits<double>;
            auto key = [](double x) { return B::key(B::raw(x)); };
            const bool an = a[i] != 0, bn = b[i] != 0;
            const bool min_b = bn && (!an || key(b[total + i]) < key(a[total + i])), max_b = bn && (!an || key(b[3 * total + i]) > key(a[3 * total + i]));
            const double w[kPlanes] = {a[i] + b[i], (min_b ? b : a)[total + i], (min_b ? b : a)[2 * total + i], (max_b ? b : a)[3 * total + i], (max_b ? b : a)[4 * total + i],
                                       a[5 * total + i] != 0 ? a[5 * total + i] : b[5 * total + i]};
            for (size_t p = 0; p < kPlanes; p++)
                if (std::memcmp(&w[p], &out[k][p * total + i], 8) != 0) return complain("continue after hold: plane " + std::to_string(p) + " element " + std::to_string(i) + " differs");
        }
        std::fill(out[k].begin(), out[k].end(), -7.0);
    }
    // a delivered call leaves an accumulator too: continue it
    if (sixdof_history_extremes(r.h, comp, 2, 3, 4, 1, wdst, 0) != SIXDOF_OK || sixdof_history_extremes(r.h, comp, 2, 7, 4, 1, wdst, kContinue) != SIXDOF_OK ||
        sixdof_history_extremes(r.h, comp, 2, 3, 8, 1, dst, 0) != SIXDOF_OK || !same_bits(out[0], want[0]) || !same_bits(out[1], want[1]))
        complain("continue after a delivered call differs from one call");
    for (int k = 0; k < 2; k++) std::fill(out[k].begin(), out[k].end(), -7.0);
    // after a call that failed in the runtime: refused, and a fresh call is correct
    if (sixdof_history_extremes(r.h, comp, 2, 3, 2, 1, nullptr, kHold) != SIXDOF_OK) complain("continue: second hold");
    hip_fake::fail_after(0);
    const int rc = sixdof_history_extremes(r.h, comp, 2, 5, 2, 1, nullptr, kHold | kContinue);
    const bool fired = hip_fake::fired();
    hip_fake::fail_after(-1);
    if (rc != SIXDOF_ERR_BACKEND || !fired) complain("continue: the injected fault did not fail the call");
    refused("after a failed call", sixdof_history_extremes(r.h, comp, 2, 7, 2, 1, dst, kContinue));
    if (sixdof_history_extremes(r.h, comp, 2, 3, 8, 1, dst, 0) != SIXDOF_OK || !same_bits(out[0], want[0]) || !same_bits(out[1], want[1])) complain("continue: the fresh call after a failed one is wrong");
    for (int k = 0; k < 2; k++) std::fill(out[k].begin(), out[k].end(), -7.0);
    // after sixdof_set_history: the ring, and the accumulator with it, are new
    if (sixdof_history_extremes(r.h, comp, 2, 3, 2, 1, nullptr, kHold) != SIXDOF_OK || sixdof_set_history(r.h, 8) != SIXDOF_OK || sixdof_step(r.h, 2, nullptr) != SIXDOF_OK)
        complain(std::string("continue: set_history: ") + sixdof_last_error(r.h));
    refused("after sixdof_set_history", sixdof_history_extremes(r.h, comp, 2, 11, 2, 1, dst, kContinue));
    if (sixdof_history_extremes(r.h, comp, 2, 11, 2, 1, dst, 0) != SIXDOF_OK || out[0][0] != 2.0) complain("continue: the fresh call on the new ring is wrong");
}

// More entries than one launch covers: 33 (the four Body names cycled, so every id repeats), each into its own buffer, in one call
// and in two; every buffer equals the buffer of the same name from a four-component read.
void more_components_than_one_launch() {
    Recorded<double> r(65, 4, 6, {true, true, false});   // the ring keeps 3 .. 6
    constexpr int kMany = 33;
    uint64_t comp[kMany];
    std::vector<double> out[kMany];
    double* dst[kMany];
    FourColumns four(65);
    if (!read_in_calls(r, four, 3, 4, 1, 1)) return complain(std::string("33 components: ") + sixdof_last_error(r.h));
    for (uint64_t segments : {uint64_t(0), uint64_t(3)}) {
        force_segments(segments);
        for (int k = 0; k < kMany; k++) comp[k] = sixdof_component_id(kNames[k % 4]), out[k].assign(kPlanes * 65 * kWidths[k % 4], -7.0), dst[k] = out[k].data();
        if (sixdof_history_extremes(r.h, comp, kMany, 3, 3, 1, nullptr, kHold) != SIXDOF_OK || sixdof_history_extremes(r.h, comp, kMany, 6, 1, 1, dst, kContinue) != SIXDOF_OK)
            return complain(std::string("33 components: ") + sixdof_last_error(r.h));
        for (int k = 0; k < kMany; k++)
            if (!same_bits(out[k], four.out[k % 4])) complain("33 components: buffer " + std::to_string(k) + " (" + kNames[k % 4] + ") differs from the four-component read");
    }
    force_segments(0);
}

// What the fault sweep reads: ticks 4, 6, 8 of world_pos and force — tick 4 held, 6 and 8 continued in two segments, so that the
// scratch, both launches and the delivery are among the calls that fail.  After every run the ring is intact.
const SweptRead kSwept{
    "extremes", {}, [](int k) { return kPlanes * 40 * (k ? 6 : 7); },
    [](sixdof_handle* h, const uint64_t* comp, void* const dst[2], bool async) {
        const int rc = sixdof_history_extremes(h, comp, 2, 4, 1, 2, nullptr, kHold);
        return rc != SIXDOF_OK ? rc : sixdof_history_extremes(h, comp, 2, 6, 2, 2, reinterpret_cast<double* const*>(dst), kContinue | (async ? SIXDOF_EXTREMES_ASYNC : 0u));
    },
    [](const Recorded<double>& r, bool fault_free, const std::vector<double> want[2], const std::string& run) {
        if (fault_free && (!same_bits(want[0], plain_loop(r, 0, 4, 3, 2)) || !same_bits(want[1], plain_loop(r, 3, 4, 3, 2)))) complain(run + ": the values are not the plain loop's");
        std::vector<double> block(40 * 7);   // tick 9 of world_pos is what was uploaded before it
        if (sixdof_history_read(r.h, sixdof_component_id("world_pos"), 9, block.data()) != SIXDOF_OK || std::memcmp(block.data(), r.truth[0][8].data(), block.size() * 8) != 0)
            complain(run + ": the ring is not what it was");
    }};

}  // namespace

int main() {
    const RecordOptions random{}, crafted{true, true, true};
    plan_arithmetic();
    values_case<double>(300, 10, 27, 18, 3, crafted);     // the range wraps the ring (slots 7 .. 9, 0 .. 6), every third tick
    values_case<float>(300, 10, 27, 18, 3, crafted);
    values_case<double>(300, 8, 9, 3, 1, crafted);        // every recorded tick: the crafted block rotates through 7 ticks
    values_case<double>(4099, 4, 5, 3, 2, random);        // a ragged last block; values that share their top bytes on world_pos
    values_case<float>(64, 8, 8, 3, 1, random);
    values_case<double>(5, 40, 42, 3, 1, crafted);        // 40 samples of few elements: the plan cuts them itself
    values_case<double>(5, 40, 42, 30, 1, random);        // 13 samples: no multiple of the load depth nor of the segment counts
    values_case<double>(1, 4, 4, 4, 1, random);           // one row, one sample
    values_case<double>(65, 4, 4, 4, 1, crafted);         // one sample: one past a wavefront
    refusals();
    continue_conditions();
    more_components_than_one_launch();
    force_segments(2);
    failure_injection("extremes_host_test", kSwept, {true, false, true});
    failure_injection("extremes_host_test", kSwept, {true, false, true}, hip_fake::kComputeFirst);
    force_segments(0);
    return verdict("extremes_host_test");
}
