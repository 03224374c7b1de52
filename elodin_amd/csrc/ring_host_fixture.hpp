// ring_host_fixture.hpp — what envelope_host_test.cpp, quantile_host_test.cpp, extremes_host_test.cpp and events_host_test.cpp
// share: the fake runtime's hooks, a recorded ring kept on the host too, and the fault sweep every reader of the ring has to
// pass whatever it computes — every fallible runtime call failed once.  For the two per-sample reductions (sixdof_capi.cpp:
// ring_bin_read) also their common refusals and more components than one launch covers; for the two scans over time
// (time_scan_read) the forced segment count and the bitwise compare.  Each program is one translation unit, so everything here
// sits in its anonymous namespace.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../../include/sixdof_hip.h"
#include "quantile_plan.hpp"

namespace hip_fake {
void fail_after(long n);
bool fired();
long calls();
long violations();
size_t live_allocations();
size_t live_streams();
size_t live_events();
size_t live_page_locks();
bool lock_intersects(const void* p, size_t bytes);   // whether any page lock intersects [p, p + bytes)
// The ordered mode (hip_fake.cpp): kAtOnce is the default, everything completes at once; under the others every stream is a queue
// that runs at forcing points only, in the order the schedule chooses where the host layer's waits leave it free.
enum { kAtOnce = 0, kMinimal = 1, kComputeFirst = 2, kCopyFirst = 3 };
void set_schedule(int schedule);
const char* schedule_name(int schedule);
size_t queued();                                      // operations enqueued and not yet run
}  // namespace hip_fake

namespace {

int g_failures = 0;
void complain(const std::string& what) {
    if (g_failures < 40) std::fprintf(stderr, "FAIL: %s\n", what.c_str());
    g_failures++;
}

// The segment count a scan is forced to through its environment variable `name`; 0: the plan's own choice again.
void force_segments(const char* name, uint64_t count) {
    if (count) setenv(name, std::to_string(count).c_str(), 1);
    else unsetenv(name);
}
bool same_bits(const std::vector<double>& a, const std::vector<double>& b) { return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0; }

const char* kNames[4] = {"world_pos", "world_vel", "world_accel", "force"};
const uint64_t kWidths[4] = {7, 6, 6, 6};

template <class T> T from_bits(uint64_t u);
template <> double from_bits<double>(uint64_t u) { double x; std::memcpy(&x, &u, 8); return x; }
template <> float from_bits<float>(uint64_t u) { const uint32_t v = static_cast<uint32_t>(u); float x; std::memcpy(&x, &v, 4); return x; }

// Element c of row r of the crafted world_vel block: one pattern per element.
template <class T>
T crafted(uint64_t r, uint64_t c, uint64_t n) {
    using L = std::numeric_limits<T>;
    const uint64_t one = sixdof::QuantileBits<T>::raw(T(1));
    const int mant = sizeof(T) == 8 ? 52 : 23;
    switch (c) {
    case 0: return T(-3.25);                                                  // all rows equal
    case 1: return r < n / 2 ? T(2.5) : T(-1.5);                              // two values in runs
    case 2: return from_bits<T>(one + (r * 37) % 251);                        // apart in the lowest byte of the mantissa only
    case 3: return from_bits<T>(((r % 2) << (sizeof(T) * 8 - 1)) | ((uint64_t(sizeof(T) == 8 ? 1000 : 100) + r % 40) << mant));   // sign and exponent only
    case 4: {
        const T v[10] = {T(-1), T(-0.0), T(0.0), L::denorm_min(), -L::denorm_min(), L::max(), L::lowest(), L::min(), T(-7.5), T(1e-30)};
        return v[(r * 7) % 10];
    }
    default:
        if (r % (n / 4 + 1) == 1) return L::quiet_NaN();                      // four NaN rows (n = 300: rows 1, 77, 153, 229)
        if (r == 5) return L::infinity();
        if (r == 6) return -L::infinity();
        return T(double(r % 17) - 8.0);
    }
}

struct RecordOptions {
    bool holes = false;         // world_vel: diverged rows and a single infinite element; force: one element that is NaN in every row
    bool crafted_vel = false;   // world_vel is the crafted block, rotated by the tick
    bool tied_force = false;    // force: few distinct values, many ties.  The random draws are the same either way.
};

// A handle of n rows whose ring holds `ticks` ticks of data that differs per tick, row and element, kept on the host too.  The
// ring is filled through the pair path, whose per-tick device copies the fake performs (f32: by the fake's recording step
// launch): before every one-tick step the host columns are rewritten and uploaded, so tick t holds what upload t carried.
template <class T>
struct Recorded {
    uint64_t n, ring, ticks;
    sixdof_handle* h = nullptr;
    std::vector<uint64_t> ids;
    std::vector<T> col[5];
    std::vector<std::vector<T>> truth[4];   // [column][tick - 1][n * w]

    Recorded(uint64_t n_, uint64_t ring_, uint64_t ticks_, RecordOptions o = {}) : n(n_), ring(ring_), ticks(ticks_) {
        std::mt19937_64 rng(n * 1000 + ring);
        std::normal_distribution<double> normal(0.0, 1.0);
        for (uint64_t i = 0; i < n; i++) ids.push_back(i + 1);
        sixdof_desc d{};
        d.struct_size = sizeof(d), d.integrator = SIXDOF_INTEGRATOR_RK4, d.simulation_time_step = 1.0 / 120.0, d.ticks_per_launch = 1;
        d.dtype = sizeof(T) == 4 ? SIXDOF_F32 : SIXDOF_F64;
        d.n_entities = n;
        std::vector<sixdof_column> cols;
        for (int k = 0; k < 5; k++) {
            const uint64_t w = k < 4 ? kWidths[k] : 7;
            col[k].assign(n * w, T(1));
            sixdof_column c{};
            c.component_id = sixdof_component_id(k < 4 ? kNames[k] : "inertia"), c.prim_type = sizeof(T) == 4 ? SIXDOF_PRIM_F32 : SIXDOF_PRIM_F64;
            c.ndim = 1, c.dims[0] = w, c.n_rows = n, c.entity_ids = ids.data(), c.host_ptr = col[k].data();
            cols.push_back(c);
        }
        const uint64_t from[1] = {1}, to[1] = {n > 1 ? 2u : 1u};
        sixdof_effector_op pair{};
        pair.kind = SIXDOF_EFF_EDGE_GRAVITY_NEWTON, pair.p[0] = 1.0;
        bool ok = sixdof_create(&d, &h) == SIXDOF_OK && sixdof_bind_columns(h, cols.data(), cols.size()) == SIXDOF_OK && sixdof_upload(h) == SIXDOF_OK;
        if (sizeof(T) == 8)   // pair effectors are f64 only: the f32 ring is filled by the (fake) step launch itself
            ok = ok && sixdof_set_edges(h, from, to, 1) == SIXDOF_OK && sixdof_set_effectors(h, &pair, 1) == SIXDOF_OK;
        for (uint64_t t = 1; ok && t <= ticks; t++) {
            if (t == 3 && ring) ok = sixdof_set_history(h, static_cast<uint32_t>(ring)) == SIXDOF_OK;   // recording starts at tick 3
            for (int k = 0; k < 4; k++) {
                for (uint64_t i = 0; i < n * kWidths[k]; i++) {
                    // world_pos: the conditioning case, values that share their top bytes: 6.4e6 plus a unit normal (f32 keeps a smaller offset apart)
                    const double offset = k == 0 ? (sizeof(T) == 4 ? 640.0 : 6.4e6) : 0.0;
                    const double x = offset + normal(rng) + 0.01 * static_cast<double>(t);
                    col[k][i] = static_cast<T>(o.tied_force && k == 3 ? std::floor(2.0 * x) : x);
                }
                if (o.crafted_vel && k == 1)
                    for (uint64_t r = 0; r < n; r++)
                        for (uint64_t c = 0; c < 6; c++) col[k][r * 6 + c] = crafted<T>((r + t) % n, c, n);
                if (o.holes && k == 1) {
                    for (uint64_t r : {uint64_t(0), n / 2, n - 1})
                        for (uint64_t c = 0; c < 6; c++) col[k][r * 6 + c] = std::numeric_limits<T>::quiet_NaN();
                    if (n > 3) col[k][1 * 6 + 2] = std::numeric_limits<T>::infinity();
                }
                if (o.holes && k == 3)
                    for (uint64_t r = 0; r < n; r++) col[k][r * 6 + 4] = std::numeric_limits<T>::quiet_NaN();
                truth[k].push_back(col[k]);
            }
            ok = ok && sixdof_upload(h) == SIXDOF_OK && sixdof_step(h, 1, nullptr) == SIXDOF_OK;
        }
        if (!ok) complain(std::string("setup: ") + (h ? sixdof_last_error(h) : sixdof_last_error(nullptr)));
    }
    ~Recorded() { sixdof_destroy(h); }
};

// One reduction read as the cases below make it: the entry point with whatever else it takes (ranks) bound by the program.
using RingRead = std::function<int(sixdof_handle* h, const uint64_t* comp, size_t n_comp, uint64_t first, uint64_t samples, uint64_t every, uint32_t period,
                                   double* const* dst, uint32_t flags)>;
using Expect = std::function<void(const char* what, int rc, int want)>;

// The refusals every reduction makes, each with a message (printed: one `refusal:` line per case) and nothing copied.  `planes`:
// the most doubles per bin `refuse` and `serve` write; `serve` makes the reads that must get as far as a launch.  own_cases(h,
// &world_pos, dst, expect): the program's own refusals, after the common argument cases; check_wide(wide, big): the values of
// the period 48 x width 6 read of world_vel.
void refusal_table(size_t planes, const RingRead& refuse, const RingRead& serve,
                   const std::function<void(sixdof_handle*, const uint64_t* pos, double* const* dst, const Expect&)>& own_cases = {},
                   const std::function<void(const Recorded<double>& wide, const std::vector<double>& big)>& check_wide = {}) {
    Recorded<double> r(24, 6, 10);   // recording since tick 3, the ring keeps 5 .. 10
    const uint64_t pos = sixdof_component_id("world_pos"), inertia = sixdof_component_id("inertia");
    std::vector<double> buf(4 * 24 * planes * 7, 123.0);
    double* dst[1] = {buf.data()};
    double* null_dst[1] = {nullptr};
    const Expect expect = [&](const char* what, int rc, int want) {
        if (rc != want) complain(std::string("refusal: ") + what + ": status " + std::to_string(rc) + ", expected " + std::to_string(want));
        else if (want != SIXDOF_OK && !*sixdof_last_error(r.h)) complain(std::string("refusal: ") + what + ": no message");
        if (want != SIXDOF_OK) std::printf("refusal: %s: %s\n", what, sixdof_last_error(r.h));
        for (double v : buf)
            if (v != 123.0) return complain(std::string("refusal: ") + what + ": something was copied"), void();
    };
    expect("every = 0", refuse(r.h, &pos, 1, 5, 2, 0, 1, dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("period = 0", refuse(r.h, &pos, 1, 5, 2, 1, 0, dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("period does not divide n", refuse(r.h, &pos, 1, 5, 2, 1, 7, dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("fallen out of the ring", refuse(r.h, &pos, 1, 4, 2, 1, 1, dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("beyond tick", refuse(r.h, &pos, 1, 9, 3, 1, 1, dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("last sample beyond tick", refuse(r.h, &pos, 1, 5, 3, 3, 1, dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("unknown flags", refuse(r.h, &pos, 1, 5, 2, 1, 1, dst, 2u), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("null buffer", refuse(r.h, &pos, 1, 5, 2, 1, 1, null_dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("null buffer list", refuse(r.h, &pos, 1, 5, 2, 1, 1, nullptr, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    if (own_cases) own_cases(r.h, &pos, dst, expect);
    expect("inertia is not recorded", refuse(r.h, &inertia, 1, 5, 2, 1, 1, dst, 0), SIXDOF_ERR_COMPONENT_NOT_FOUND);
    expect("no samples", refuse(r.h, &pos, 1, 99, 0, 7, 1, dst, 0), SIXDOF_OK);
    if (serve(r.h, &pos, 1, 5, 4, 1, 24, dst, 0) != SIXDOF_OK || buf.back() == 123.0) complain("one row per group (period = n) is refused or fills nothing");
    std::fill(buf.begin(), buf.end(), 123.0);
    if (sixdof_set_history(r.h, 0) != SIXDOF_OK) complain("refusal: set_history(0)");
    expect("no ring", refuse(r.h, &pos, 1, 5, 2, 1, 1, dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    // the width limit: 96 rows in groups of 96 are 672 bins of world_pos, 576 of world_vel; 48 x 6 = 288 are served
    Recorded<double> wide(96, 4, 4);
    const uint64_t vel = sixdof_component_id("world_vel");
    std::vector<double> big(1 * 96 * planes * 6, 123.0);
    double* bdst[1] = {big.data()};
    const int rc = serve(wide.h, &vel, 1, 4, 1, 1, 96, bdst, 0);
    if (rc != SIXDOF_ERR_INVALID_ARGUMENT || !std::strstr(sixdof_last_error(wide.h), "512")) complain("refusal: period x width beyond the limit is not refused with the limit named");
    std::printf("refusal: %s: %s\n", "period x width beyond the limit", sixdof_last_error(wide.h));
    for (double v : big)
        if (v != 123.0) return complain("refusal: period x width beyond the limit: something was copied");
    if (serve(wide.h, &vel, 1, 4, 1, 1, 48, bdst, 0) != SIXDOF_OK) complain(std::string("period 48 x width 6: ") + sixdof_last_error(wide.h));
    if (check_wide) check_wide(wide, big);
}

// More components than one launch covers: 34 (the four Body names cycled) of a 65-row world in 5 groups, two samples, each into
// its own buffer — the second launch reuses the scratch offsets of the first.  Every buffer equals, bitwise, the buffer of the
// same name from a four-component read.
void more_components_than_one_launch_covers(size_t planes, const RingRead& read, RecordOptions o = {}) {
    Recorded<double> r(65, 4, 4, o);   // recording since tick 3: samples 3 and 4
    constexpr int kMany = 34;
    uint64_t comp[kMany];
    std::vector<double> out[kMany], want[4];
    double *dst[kMany], *wdst[4];
    for (int k = 0; k < kMany; k++) comp[k] = sixdof_component_id(kNames[k % 4]), out[k].assign(2 * 5 * planes * kWidths[k % 4], -7.0), dst[k] = out[k].data();
    for (int k = 0; k < 4; k++) want[k].assign(out[k].size(), -9.0), wdst[k] = want[k].data();
    if (read(r.h, comp, kMany, 3, 2, 1, 5, dst, 0) != SIXDOF_OK || read(r.h, comp, 4, 3, 2, 1, 5, wdst, 0) != SIXDOF_OK)
        return complain(std::string("34 components: ") + sixdof_last_error(r.h));
    for (int k = 0; k < kMany; k++)
        if (want[k % 4].back() == -9.0 || std::memcmp(out[k].data(), want[k % 4].data(), out[k].size() * sizeof(double)) != 0)
            complain("34 components: buffer " + std::to_string(k) + " (" + kNames[k % 4] + ") differs from the four-component read");
}

// What a fault sweep reads: ticks 4, 6, 8 of world_pos and force of a 40-row ring with holes.
struct SweptRead {
    const char* name;
    std::function<int(sixdof_handle*, const uint64_t comp[2])> setup;                      // before the fault is armed
    std::function<size_t(int k)> doubles;
    std::function<int(sixdof_handle*, const uint64_t comp[2], void* const dst[2], bool async)> read;
    // after every run, the handle still alive: `want` is the fault-free run's blocking read (that run itself: fault_free)
    std::function<void(const Recorded<double>& r, bool fault_free, const std::vector<double> want[2], const std::string& run)> check;
};

// Each fallible runtime call of a blocking and of an asynchronous read is failed once: the status is returned with a message,
// the call succeeds when repeated, its values are the fault-free run's, and nothing outlives the handle.  Under a lazy `schedule`
// a fault in a deferred operation is reported by the forcing point that reaches it, which may be a later step than the call
// that enqueued it: still exactly one step reports it.
void failure_injection(const char* program, const SweptRead& swept, RecordOptions o, int schedule = hip_fake::kAtOnce) {
    hip_fake::set_schedule(schedule);
    const uint64_t comp[2] = {sixdof_component_id("world_pos"), sixdof_component_id("force")};
    std::vector<double> want[2];
    long n_calls = 0;
    for (long fault = -1; fault < n_calls || fault < 0; fault++) {
        const std::string run = std::string(swept.name) + ": fault at call " + std::to_string(fault);
        {
            Recorded<double> r(40, 8, 9, o);
            if (swept.setup && swept.setup(r.h, comp) != SIXDOF_OK) complain(run + ": setup: " + sixdof_last_error(r.h));
            std::vector<double> out[2][2];
            int failed = 0;
            const long calls0 = hip_fake::calls();
            hip_fake::fail_after(fault);
            for (int a = 0; a < 2; a++) {   // blocking, then asynchronous: the second grows neither buffer
                void* dst[2];
                for (int k = 0; k < 2; k++) out[a][k].assign(swept.doubles(k), -1.0), dst[k] = out[a][k].data();
                auto read = [&] { return swept.read(r.h, comp, dst, a != 0); };
                int rc = read();
                if (rc != SIXDOF_OK) {
                    if (!hip_fake::fired() || failed || !*sixdof_last_error(r.h)) complain(run + ": a read failed with no fault of the test's behind it: " + sixdof_last_error(r.h));
                    failed++;
                    if (rc != SIXDOF_ERR_BACKEND) complain(run + ": status " + std::to_string(rc));
                    if (read() != SIXDOF_OK) complain(run + ": the read fails again without a fault: " + sixdof_last_error(r.h));
                }
            }
            int rc = sixdof_download_wait(r.h);
            if (rc != SIXDOF_OK && (failed++, sixdof_download_wait(r.h) != SIXDOF_OK)) complain(run + ": download_wait");
            rc = sixdof_sync(r.h);
            if (rc != SIXDOF_OK && (failed++, sixdof_sync(r.h) != SIXDOF_OK)) complain(run + ": sync");
            hip_fake::fail_after(-1);
            if (fault < 0) {
                n_calls = hip_fake::calls() - calls0;
                for (int k = 0; k < 2; k++) want[k] = out[0][k];
                if (failed) complain("fault-free run failed");
            } else if (failed != 1) {
                complain(run + ": " + std::to_string(failed) + " steps reported it");
            }
            for (int a = 0; a < 2; a++)
                for (int k = 0; k < 2; k++)
                    if (std::memcmp(out[a][k].data(), want[k].data(), want[k].size() * sizeof(double)) != 0) complain(run + ": the values after the retry differ from the fault-free run's");
            if (swept.check) swept.check(r, fault < 0, want, run);
        }
        if (hip_fake::live_allocations() || hip_fake::live_streams() || hip_fake::live_events() || hip_fake::live_page_locks()) complain(run + ": something outlives sixdof_destroy");
    }
    hip_fake::set_schedule(hip_fake::kAtOnce);
    if (schedule == hip_fake::kAtOnce) std::printf("%s: %ld fallible calls of a blocking and an asynchronous %s read, each failed once\n", program, n_calls, swept.name);
    else std::printf("%s: under the %s schedule: %ld fallible calls of the same %s reads, each failed once\n", program, hip_fake::schedule_name(schedule), n_calls, swept.name);
}

// The end of a program's main: the fake runtime's own findings, the verdict line, the exit status.
int verdict(const char* program) {
    if (hip_fake::violations()) complain(std::to_string(hip_fake::violations()) + " violations reported by the fake runtime");
    if (g_failures) return std::fprintf(stderr, "%s: %d failures\n", program, g_failures), 1;
    std::printf("%s: ok\n", program);
    return 0;
}

}  // namespace
