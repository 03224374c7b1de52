// envelope_host_test.cpp — sixdof_history_envelope (sixdof_capi.cpp) over the fake runtime (hip_fake.cpp), whose launcher computes
// the real reduction through envelope_plan.hpp in the kernels' geometry and merge order, under AddressSanitizer / UBSan, no GPU:
// `make envelope_test`, tests/test_history_envelope_host.py.
//
// The ring is filled through the pair path, whose per-tick device copies the fake performs (f32: by the fake's recording step
// launch): before every one-tick step the host columns are rewritten and uploaded, so tick t holds what upload t carried.  Checked: the values against a long-double
// two-pass reference, every refusal with nothing copied, bit-identity of a range's samples with single-sample reads, and
// every fallible runtime call of the entry point failed once.  The readers that share its copy lane and staging rules ride
// along: sixdof_watch_read in the same fault sweep, both pending on one lane, sixdof_history_stream across the ring's wrap.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../../include/sixdof_hip.h"
#include "envelope_plan.hpp"

namespace hip_fake {
void fail_after(long n);
bool fired();
long calls();
long violations();
size_t live_allocations();
size_t live_streams();
size_t live_events();
size_t live_page_locks();
}  // namespace hip_fake

namespace {

int g_failures = 0;
void complain(const std::string& what) {
    std::fprintf(stderr, "FAIL: %s\n", what.c_str());
    g_failures++;
}

const char* kNames[4] = {"world_pos", "world_vel", "world_accel", "force"};
const uint64_t kWidths[4] = {7, 6, 6, 6};

// A handle of n rows whose ring holds `ticks` ticks of data that differs per tick, row and element, kept on the host too.
template <class T>
struct Recorded {
    uint64_t n, ring, ticks;
    sixdof_handle* h = nullptr;
    std::vector<uint64_t> ids;
    std::vector<T> col[5];
    std::vector<std::vector<T>> truth[4];   // [column][tick - 1][n * w]

    Recorded(uint64_t n_, uint64_t ring_, uint64_t ticks_, bool holes) : n(n_), ring(ring_), ticks(ticks_) {
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
                    // world_pos: the conditioning case, 6.4e6 plus a unit normal (f32 keeps a smaller offset apart)
                    const double offset = k == 0 ? (sizeof(T) == 4 ? 640.0 : 6.4e6) : 0.0;
                    col[k][i] = static_cast<T>(offset + normal(rng) + 0.01 * static_cast<double>(t));
                }
                if (holes && k == 1) {   // diverged rows, a single infinite element, and one column that is NaN in every row
                    for (uint64_t r : {uint64_t(0), n / 2, n - 1})
                        for (uint64_t c = 0; c < 6; c++) col[k][r * 6 + c] = std::numeric_limits<T>::quiet_NaN();
                    if (n > 3) col[k][1 * 6 + 2] = std::numeric_limits<T>::infinity();
                }
                if (holes && k == 3)
                    for (uint64_t r = 0; r < n; r++) col[k][r * 6 + 4] = std::numeric_limits<T>::quiet_NaN();
                truth[k].push_back(col[k]);
            }
            ok = ok && sixdof_upload(h) == SIXDOF_OK && sixdof_step(h, 1, nullptr) == SIXDOF_OK;
        }
        if (!ok) complain(std::string("setup: ") + (h ? sixdof_last_error(h) : sixdof_last_error(nullptr)));
    }
    ~Recorded() { sixdof_destroy(h); }
};

size_t out_doubles(uint64_t n_samples, uint32_t period, uint64_t w) { return n_samples * period * 5 * w; }

// values of one read against the two-pass long-double reference, with the bounds the GPU tests use
template <class T>
void check_values(const Recorded<T>& r, int k, uint64_t first, uint64_t n_samples, uint64_t every, uint32_t period, const std::vector<double>& got,
                  const std::string& what) {
    const uint64_t w = kWidths[k];
    const double eps = std::numeric_limits<double>::epsilon();
    for (uint64_t j = 0; j < n_samples; j++) {
        const std::vector<T>& x = r.truth[k][first + j * every - 1];
        for (uint32_t g = 0; g < period; g++)
            for (uint64_t c = 0; c < w; c++) {
                long double sum = 0, sum_abs = 0, m2 = 0;
                double mn = INFINITY, mx = -INFINITY, cnt = 0;
                for (uint64_t row = g; row < r.n; row += period) {
                    const double v = static_cast<double>(x[row * w + c]);
                    if (!std::isfinite(v)) continue;
                    cnt += 1, sum += v, sum_abs += std::fabs(v), mn = std::fmin(mn, v), mx = std::fmax(mx, v);
                }
                const long double mean = cnt ? sum / cnt : 0;
                for (uint64_t row = g; row < r.n; row += period) {
                    const double v = static_cast<double>(x[row * w + c]);
                    if (std::isfinite(v)) m2 += (v - mean) * (v - mean);
                }
                const double* o = &got[((j * period + g) * 5) * w + c];
                const std::string at = what + ": " + kNames[k] + " sample " + std::to_string(j) + " group " + std::to_string(g) + " element " + std::to_string(c);
                if (o[0] != cnt) complain(at + ": count " + std::to_string(o[0]) + " != " + std::to_string(cnt));
                if (cnt == 0) {
                    for (int s = 1; s < 5; s++)
                        if (!std::isnan(o[s * w])) complain(at + ": statistic " + std::to_string(s) + " of an empty group is not NaN");
                    continue;
                }
                if (o[w] != mn || o[2 * w] != mx) complain(at + ": min / max");
                const double mean_bound = 2 * cnt * eps * static_cast<double>(sum_abs / cnt);
                if (!(std::fabs(static_cast<double>(o[3 * w] - mean)) <= mean_bound)) complain(at + ": mean off by " + std::to_string(static_cast<double>(o[3 * w] - mean)));
                const double kappa = m2 > 0 ? std::sqrt(1.0 + cnt * static_cast<double>(mean * mean / m2)) : 1.0;
                const double m2_bound = cnt * eps * kappa * static_cast<double>(m2);
                if (!(std::fabs(static_cast<double>(o[4 * w] - m2)) <= m2_bound))
                    complain(at + ": m2 " + std::to_string(o[4 * w]) + " against " + std::to_string(static_cast<double>(m2)) + ", bound " + std::to_string(m2_bound));
            }
    }
}

template <class T>
void values_case(uint64_t n, uint64_t ring, uint64_t ticks, uint64_t first, uint64_t every, uint32_t period, bool holes) {
    Recorded<T> r(n, ring, ticks, holes);
    const std::string what = std::string(sizeof(T) == 4 ? "f32" : "f64") + " n " + std::to_string(n) + " period " + std::to_string(period);
    const uint64_t n_samples = (ticks - first) / every + 1;
    uint64_t comp[4];
    std::vector<double> out[4];
    double* dst[4];
    for (int k = 0; k < 4; k++) comp[k] = sixdof_component_id(kNames[k]), out[k].assign(out_doubles(n_samples, period, kWidths[k]), -7.0), dst[k] = out[k].data();
    if (sixdof_history_envelope(r.h, comp, 4, first, n_samples, every, period, dst, 0) != SIXDOF_OK) return complain(what + ": " + sixdof_last_error(r.h));
    for (int k = 0; k < 4; k++) check_values(r, k, first, n_samples, every, period, out[k], what);
    // bit-identity: every sample equals the single-sample read of its tick, alone and in another component list
    for (uint64_t j = 0; j < n_samples; j++)
        for (int k = 0; k < 4; k++) {
            std::vector<double> one(out_doubles(1, period, kWidths[k]), -7.0), other(out_doubles(1, period, kWidths[(k + 1) % 4]));
            double* d1[2] = {other.data(), one.data()};
            const uint64_t c2[2] = {comp[(k + 1) % 4], comp[k]};
            if (sixdof_history_envelope(r.h, c2, 2, first + j * every, 1, 5, period, d1, j % 2 ? SIXDOF_ENVELOPE_ASYNC : 0u) != SIXDOF_OK || sixdof_download_wait(r.h) != SIXDOF_OK)
                return complain(what + ": single-sample read: " + sixdof_last_error(r.h));
            if (std::memcmp(one.data(), &out[k][j * one.size()], one.size() * sizeof(double)) != 0)
                complain(what + ": " + kNames[k] + " sample " + std::to_string(j) + " of the range differs from the single-sample read of its tick");
        }
    if (sixdof_sync(r.h) != SIXDOF_OK) complain(what + ": sync");
}

void refusals() {
    Recorded<double> r(24, 6, 10, false);   // recording since tick 3, the ring keeps 5 .. 10
    const uint64_t pos = sixdof_component_id("world_pos"), inertia = sixdof_component_id("inertia");
    std::vector<double> buf(out_doubles(4, 24, 7), 123.0);
    double* dst[1] = {buf.data()};
    double* null_dst[1] = {nullptr};
    auto expect = [&](const char* what, int rc, int want) {
        if (rc != want) complain(std::string("refusal: ") + what + ": status " + std::to_string(rc) + ", expected " + std::to_string(want));
        else if (want != SIXDOF_OK && !*sixdof_last_error(r.h)) complain(std::string("refusal: ") + what + ": no message");
        for (double v : buf)
            if (v != 123.0) return complain(std::string("refusal: ") + what + ": something was copied"), void();
    };
    expect("every = 0", sixdof_history_envelope(r.h, &pos, 1, 5, 2, 0, 1, dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("period = 0", sixdof_history_envelope(r.h, &pos, 1, 5, 2, 1, 0, dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("period does not divide n", sixdof_history_envelope(r.h, &pos, 1, 5, 2, 1, 7, dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("fallen out of the ring", sixdof_history_envelope(r.h, &pos, 1, 4, 2, 1, 1, dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("beyond tick", sixdof_history_envelope(r.h, &pos, 1, 9, 3, 1, 1, dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("last sample beyond tick", sixdof_history_envelope(r.h, &pos, 1, 5, 3, 3, 1, dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("unknown flags", sixdof_history_envelope(r.h, &pos, 1, 5, 2, 1, 1, dst, 2u), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("null buffer", sixdof_history_envelope(r.h, &pos, 1, 5, 2, 1, 1, null_dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("null buffer list", sixdof_history_envelope(r.h, &pos, 1, 5, 2, 1, 1, nullptr, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("inertia is not recorded", sixdof_history_envelope(r.h, &inertia, 1, 5, 2, 1, 1, dst, 0), SIXDOF_ERR_COMPONENT_NOT_FOUND);
    expect("no samples", sixdof_history_envelope(r.h, &pos, 1, 99, 0, 7, 1, dst, 0), SIXDOF_OK);
    if (sixdof_history_envelope(r.h, &pos, 1, 5, 4, 1, 24, dst, 0) != SIXDOF_OK || buf.back() == 123.0) complain("one row per group (period = n) is refused or fills nothing");
    std::fill(buf.begin(), buf.end(), 123.0);
    if (sixdof_set_history(r.h, 0) != SIXDOF_OK) complain("refusal: set_history(0)");
    expect("no ring", sixdof_history_envelope(r.h, &pos, 1, 5, 2, 1, 1, dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    // the width limit: 96 rows in groups of 96 are 672 bins of world_pos, 576 of world_vel
    Recorded<double> wide(96, 4, 4, false);
    const uint64_t vel = sixdof_component_id("world_vel");
    std::vector<double> big(out_doubles(1, 96, 7), 123.0);
    double* bdst[1] = {big.data()};
    int rc = sixdof_history_envelope(wide.h, &vel, 1, 4, 1, 1, 96, bdst, 0);
    if (rc != SIXDOF_ERR_INVALID_ARGUMENT || !std::strstr(sixdof_last_error(wide.h), "512")) complain("refusal: period x width beyond the limit is not refused with the limit named");
    for (double v : big)
        if (v != 123.0) return complain("refusal: period x width beyond the limit: something was copied");
    if (sixdof_history_envelope(wide.h, &vel, 1, 4, 1, 1, 48, bdst, 0) != SIXDOF_OK) complain(std::string("period 48 x width 6: ") + sixdof_last_error(wide.h));
}

// Two staged readers pending on one copy lane: an asynchronous watch read, an asynchronous envelope read behind it and — with
// `regrow` — a second, larger watch read whose staging buffer has to grow while the first two are pending, then ONE
// sixdof_download_wait.  Everything equals the blocking reads of the same ranges byte for byte, and sixdof_sync ends the page locks.
void two_readers_one_lane(bool regrow) {
    const std::string what = regrow ? "two readers, staging regrown while pending" : "two readers on one lane";
    Recorded<double> r(24, 4, 6, false);   // recording since tick 3: the ring of 4 holds 3 .. 6, tick 5 in slot 0
    const uint64_t comp[2] = {sixdof_component_id("world_pos"), sixdof_component_id("world_vel")}, who[3] = {1, 12, 24};
    if (sixdof_set_watch(r.h, comp, 2, who, 3) != SIXDOF_OK) return complain(what + ": set_watch: " + sixdof_last_error(r.h));
    // [0] watch 3, 5   [1] envelope 4, 5, 6 in two groups   [2] watch 3 .. 6;   [.][0] asynchronous, [.][1] blocking
    std::vector<double> out[3][2][2];
    auto read = [&](int which, int blocking) {
        const uint64_t samples = which == 0 ? 2 : which == 1 ? 3 : 4;
        void* dst[2];
        for (int k = 0; k < 2; k++) {
            out[which][blocking][k].assign(which == 1 ? out_doubles(samples, 2, kWidths[k]) : 3 * samples * kWidths[k], -7.0);
            dst[k] = out[which][blocking][k].data();
        }
        const int rc = which == 1 ? sixdof_history_envelope(r.h, comp, 2, 4, samples, 1, 2, reinterpret_cast<double**>(dst), blocking ? 0u : SIXDOF_ENVELOPE_ASYNC)
                                  : sixdof_watch_read(r.h, 3, samples, which == 0 ? 2 : 1, dst, blocking ? 0u : SIXDOF_WATCH_ASYNC);
        if (rc != SIXDOF_OK) complain(what + ": read " + std::to_string(which) + ": " + sixdof_last_error(r.h));
    };
    const int n_reads = regrow ? 3 : 2;
    for (int which = 0; which < n_reads; which++) read(which, 0);
    if (sixdof_download_wait(r.h) != SIXDOF_OK || sixdof_sync(r.h) != SIXDOF_OK) complain(what + ": download_wait / sync: " + sixdof_last_error(r.h));
    if (hip_fake::live_page_locks()) complain(what + ": " + std::to_string(hip_fake::live_page_locks()) + " page locks are alive after sixdof_sync");
    for (int which = 0; which < n_reads; which++) {
        read(which, 1);
        for (int k = 0; k < 2; k++) {
            const std::vector<double>&got = out[which][0][k], &want = out[which][1][k];
            if (std::memcmp(got.data(), want.data(), want.size() * sizeof(double)) != 0) complain(what + ": read " + std::to_string(which) + " differs from the blocking read of its range");
            if (want[0] == -7.0 || want.back() == -7.0) complain(what + ": the blocking read " + std::to_string(which) + " filled nothing");
        }
    }
    // the watch read is the ring's rows themselves: entity 12 (row 11), tick 5 is sample 1 of read 0
    if (std::memcmp(&out[0][0][0][(1 * 2 + 1) * 7], &r.truth[0][5 - 1][11 * 7], 7 * sizeof(double)) != 0) complain(what + ": the watch read is not what was uploaded before tick 5");
}

// sixdof_history_stream across the ring's wrap: ticks 3 .. 6 of a ring of 4 (slots 2 3 0 1) equal four sixdof_history_reads.
void stream_across_the_wrap() {
    Recorded<double> r(24, 4, 6, false);
    std::vector<double> run[4], one;
    void* dst[4];
    for (int k = 0; k < 4; k++) run[k].assign(4 * r.n * kWidths[k], -7.0), dst[k] = run[k].data();
    if (sixdof_history_stream(r.h, 3, 4, dst) != SIXDOF_OK || sixdof_download_wait(r.h) != SIXDOF_OK) return complain(std::string("history_stream across the wrap: ") + sixdof_last_error(r.h));
    for (int k = 0; k < 4; k++)
        for (uint64_t t = 3; t <= 6; t++) {
            one.assign(r.n * kWidths[k], -9.0);
            if (sixdof_history_read(r.h, sixdof_component_id(kNames[k]), t, one.data()) != SIXDOF_OK) return complain(std::string("history_read: ") + sixdof_last_error(r.h));
            if (std::memcmp(&run[k][(t - 3) * one.size()], one.data(), one.size() * sizeof(double)) != 0)
                complain(std::string("history_stream across the wrap: ") + kNames[k] + " tick " + std::to_string(t) + " differs from history_read");
            if (std::memcmp(one.data(), r.truth[k][t - 1].data(), one.size() * sizeof(double)) != 0)
                complain(std::string("history_read: ") + kNames[k] + " tick " + std::to_string(t) + " is not what was uploaded before it");
        }
    const uint64_t top = ~uint64_t(0);
    if (sixdof_history_stream(r.h, 2, top, dst) != SIXDOF_ERR_INVALID_ARGUMENT || sixdof_history_stream(r.h, 3, 5, dst) != SIXDOF_ERR_INVALID_ARGUMENT ||
        sixdof_history_stream(r.h, 2, 4, dst) != SIXDOF_ERR_INVALID_ARGUMENT || sixdof_history_read(r.h, sixdof_component_id("force"), 7, one.data()) != SIXDOF_ERR_INVALID_ARGUMENT)
        complain("history_stream / history_read accept ticks that are not in the ring");
    if (sixdof_sync(r.h) != SIXDOF_OK) complain("history_stream across the wrap: sync");
}

// What the fault sweep reads: ticks 4, 6, 8 of world_pos and force, as envelopes in four groups or as the watched rows.
struct SweptRead {
    const char* name;
    int (*setup)(sixdof_handle*, const uint64_t comp[2]);                      // before the fault is armed
    size_t (*doubles)(int k);
    int (*read)(sixdof_handle*, const uint64_t comp[2], void* const dst[2], bool async);
};
const uint64_t kSweptEntities[3] = {1, 17, 40};
const SweptRead kSweptReads[2] = {
    {"envelope", [](sixdof_handle*, const uint64_t*) { return int(SIXDOF_OK); }, [](int k) { return out_doubles(3, 4, k ? 6 : 7); },
     [](sixdof_handle* h, const uint64_t* comp, void* const dst[2], bool async) {
         return sixdof_history_envelope(h, comp, 2, 4, 3, 2, 4, reinterpret_cast<double* const*>(dst), async ? SIXDOF_ENVELOPE_ASYNC : 0u);
     }},
    {"watch", [](sixdof_handle* h, const uint64_t* comp) { return sixdof_set_watch(h, comp, 2, kSweptEntities, 3); }, [](int k) { return size_t(3 * 3 * (k ? 6 : 7)); },
     [](sixdof_handle* h, const uint64_t*, void* const dst[2], bool async) { return sixdof_watch_read(h, 4, 3, 2, dst, async ? SIXDOF_WATCH_ASYNC : 0u); }},
};

// Each fallible runtime call of a blocking and of an asynchronous read is failed once: the status is returned with a message,
// the call succeeds when repeated, its values are the fault-free run's, and nothing outlives the handle.
void failure_injection(const SweptRead& swept) {
    const uint64_t comp[2] = {sixdof_component_id("world_pos"), sixdof_component_id("force")};
    std::vector<double> want[2];
    long n_calls = 0;
    for (long fault = -1; fault < n_calls || fault < 0; fault++) {
        const std::string run = std::string(swept.name) + ": fault at call " + std::to_string(fault);
        {
            Recorded<double> r(40, 8, 9, true);
            if (swept.setup(r.h, comp) != SIXDOF_OK) complain(run + ": setup: " + sixdof_last_error(r.h));
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
                if (want[0][0] == -1.0 || want[1].back() == -1.0) complain(run + ": the fault-free read filled nothing");
            } else if (failed != 1) {
                complain(run + ": " + std::to_string(failed) + " steps reported it");
            }
            for (int a = 0; a < 2; a++)
                for (int k = 0; k < 2; k++)
                    if (std::memcmp(out[a][k].data(), want[k].data(), want[k].size() * sizeof(double)) != 0) complain(run + ": the values after the retry differ from the fault-free run's");
        }
        if (hip_fake::live_allocations() || hip_fake::live_streams() || hip_fake::live_events() || hip_fake::live_page_locks()) complain(run + ": something outlives sixdof_destroy");
    }
    std::printf("envelope_host_test: %ld fallible calls of a blocking and an asynchronous %s read, each failed once\n", n_calls, swept.name);
}

}  // namespace

int main() {
    values_case<double>(300, 10, 27, 18, 3, 1, true);     // the range wraps the ring; diverged rows
    values_case<double>(4099, 4, 5, 3, 2, 1, false);      // several blocks, a ragged last tile; the conditioning case on world_pos
    values_case<double>(300, 8, 9, 9, 1, 12, true);       // groups
    values_case<double>(320, 4, 5, 4, 1, 64, false);      // a wavefront-sized world: 448 bins of world_pos
    values_case<float>(64, 8, 8, 3, 1, 1, true);
    values_case<double>(1, 4, 4, 4, 1, 1, false);
    values_case<double>(65, 4, 4, 3, 1, 5, false);
    refusals();
    two_readers_one_lane(false);
    two_readers_one_lane(true);
    stream_across_the_wrap();
    for (const SweptRead& swept : kSweptReads) failure_injection(swept);
    if (hip_fake::violations()) complain(std::to_string(hip_fake::violations()) + " violations reported by the fake runtime");
    if (g_failures) return std::fprintf(stderr, "envelope_host_test: %d failures\n", g_failures), 1;
    std::printf("envelope_host_test: ok\n");
    return 0;
}
