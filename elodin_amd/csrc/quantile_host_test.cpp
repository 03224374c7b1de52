// quantile_host_test.cpp — sixdof_history_quantiles (sixdof_capi.cpp) over the fake runtime (hip_fake.cpp), whose launcher selects
// through quantile_plan.hpp's keys, scan step and lo -> hi rule, under AddressSanitizer / UBSan, no GPU: `make quantile_test`,
// tests/test_history_quantiles_host.py.
//
// The ring is filled as in envelope_host_test.cpp: before every one-tick step the host columns are rewritten and uploaded, so
// tick t holds what upload t carried.  Checked: every value bitwise against std::sort on the keys, over random and crafted
// blocks (ties, runs, values apart in the lowest byte only or in sign and exponent only, +-0, denormals, +-max, NaN, +-inf),
// every refusal with nothing copied, bit-identity of a range's samples with single-sample reads, a range long enough to be cut
// into several launches, and every fallible runtime call of the entry point failed once.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
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
}  // namespace hip_fake

namespace {

using sixdof::QuantileBits;

int g_failures = 0;
void complain(const std::string& what) {
    if (g_failures < 40) std::fprintf(stderr, "FAIL: %s\n", what.c_str());
    g_failures++;
}

const char* kNames[4] = {"world_pos", "world_vel", "world_accel", "force"};
const uint64_t kWidths[4] = {7, 6, 6, 6};

template <class T> T from_bits(uint64_t u);
template <> double from_bits<double>(uint64_t u) { double x; std::memcpy(&x, &u, 8); return x; }
template <> float from_bits<float>(uint64_t u) { const uint32_t v = static_cast<uint32_t>(u); float x; std::memcpy(&x, &v, 4); return x; }

// Element c of row r of the crafted world_vel block: one pattern per element.
template <class T>
T crafted(uint64_t r, uint64_t c, uint64_t n) {
    using L = std::numeric_limits<T>;
    const uint64_t one = QuantileBits<T>::raw(T(1));
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

// A handle of n rows whose ring holds `ticks` ticks of data that differs per tick, row and element, kept on the host too.
template <class T>
struct Recorded {
    uint64_t n, ring, ticks;
    sixdof_handle* h = nullptr;
    std::vector<uint64_t> ids;
    std::vector<T> col[5];
    std::vector<std::vector<T>> truth[4];   // [column][tick - 1][n * w]

    // holes: diverged rows and an all-NaN element as in envelope_host_test.cpp; craft: world_vel is the crafted block
    Recorded(uint64_t n_, uint64_t ring_, uint64_t ticks_, bool holes, bool craft = false) : n(n_), ring(ring_), ticks(ticks_) {
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
                    // world_pos: values that share their top bytes, 6.4e6 plus a unit normal; force: few distinct values, many ties
                    const double offset = k == 0 ? (sizeof(T) == 4 ? 640.0 : 6.4e6) : 0.0;
                    const double x = offset + normal(rng) + 0.01 * static_cast<double>(t);
                    col[k][i] = static_cast<T>(k == 3 ? std::floor(2.0 * x) : x);
                }
                if (craft && k == 1)
                    for (uint64_t r = 0; r < n; r++)
                        for (uint64_t c = 0; c < 6; c++) col[k][r * 6 + c] = crafted<T>((r + t) % n, c, n);
                if (holes && k == 1) {   // diverged rows, a single infinite element
                    for (uint64_t r : {uint64_t(0), n / 2, n - 1})
                        for (uint64_t c = 0; c < 6; c++) col[k][r * 6 + c] = std::numeric_limits<T>::quiet_NaN();
                    if (n > 3) col[k][1 * 6 + 2] = std::numeric_limits<T>::infinity();
                }
                if (holes && k == 3)     // one element that is NaN in every row
                    for (uint64_t r = 0; r < n; r++) col[k][r * 6 + 4] = std::numeric_limits<T>::quiet_NaN();
                truth[k].push_back(col[k]);
            }
            ok = ok && sixdof_upload(h) == SIXDOF_OK && sixdof_step(h, 1, nullptr) == SIXDOF_OK;
        }
        if (!ok) complain(std::string("setup: ") + (h ? sixdof_last_error(h) : sixdof_last_error(nullptr)));
    }
    ~Recorded() { sixdof_destroy(h); }
};

struct Ranks {
    std::vector<uint32_t> num;
    uint32_t den;
};
size_t out_doubles(uint64_t n_samples, uint32_t period, uint64_t w, size_t n_ranks) { return n_samples * period * (1 + 2 * n_ranks) * w; }

// one read against std::sort on the keys, bit for bit
template <class T>
void check_values(const Recorded<T>& r, int k, uint64_t first, uint64_t n_samples, uint64_t every, uint32_t period, const Ranks& q,
                  const std::vector<double>& got, const std::string& what) {
    using B = QuantileBits<T>;
    const uint64_t w = kWidths[k], planes = 1 + 2 * q.num.size();
    std::vector<uint64_t> keys;
    for (uint64_t j = 0; j < n_samples; j++) {
        const std::vector<T>& x = r.truth[k][first + j * every - 1];
        for (uint32_t g = 0; g < period; g++)
            for (uint64_t c = 0; c < w; c++) {
                keys.clear();
                for (uint64_t row = g; row < r.n; row += period)
                    if (std::isfinite(x[row * w + c])) keys.push_back(B::key(B::raw(x[row * w + c])));
                std::sort(keys.begin(), keys.end());
                const double* o = &got[((j * period + g) * planes) * w + c];
                const std::string at = what + ": " + kNames[k] + " sample " + std::to_string(j) + " group " + std::to_string(g) + " element " + std::to_string(c);
                if (o[0] != static_cast<double>(keys.size())) complain(at + ": count " + std::to_string(o[0]) + " != " + std::to_string(keys.size()));
                for (size_t i = 0; i < q.num.size(); i++) {
                    double want[2] = {std::nan(""), std::nan("")};
                    if (!keys.empty()) {
                        const uint64_t p = uint64_t(q.num[i]) * (keys.size() - 1);
                        want[0] = B::value(keys[p / q.den]), want[1] = B::value(keys[(p + q.den - 1) / q.den]);
                    }
                    for (int s = 0; s < 2; s++) {
                        const double have = o[(1 + 2 * i + s) * w];
                        if (keys.empty() ? !std::isnan(have) : std::memcmp(&have, &want[s], 8) != 0)
                            complain(at + ": rank " + std::to_string(q.num[i]) + "/" + std::to_string(q.den) + (s ? " upper " : " lower ") + std::to_string(have) + " != " + std::to_string(want[s]));
                    }
                }
            }
    }
}

template <class T>
void values_case(uint64_t n, uint64_t ring, uint64_t ticks, uint64_t first, uint64_t every, uint32_t period, bool holes, const Ranks& q, bool craft = false) {
    Recorded<T> r(n, ring, ticks, holes, craft);
    const std::string what = std::string(sizeof(T) == 4 ? "f32" : "f64") + " n " + std::to_string(n) + " period " + std::to_string(period) + " ranks " + std::to_string(q.num.size());
    const uint64_t n_samples = (ticks - first) / every + 1;
    const size_t R = q.num.size();
    uint64_t comp[4];
    std::vector<double> out[4];
    double* dst[4];
    for (int k = 0; k < 4; k++) comp[k] = sixdof_component_id(kNames[k]), out[k].assign(out_doubles(n_samples, period, kWidths[k], R), -7.0), dst[k] = out[k].data();
    if (sixdof_history_quantiles(r.h, comp, 4, first, n_samples, every, period, q.num.data(), q.den, R, dst, 0) != SIXDOF_OK) return complain(what + ": " + sixdof_last_error(r.h));
    for (int k = 0; k < 4; k++) check_values(r, k, first, n_samples, every, period, q, out[k], what);
    // bit-identity: every sample equals the single-sample read of its tick, in another component list, alone or asynchronous
    for (uint64_t j = 0; j < n_samples; j++)
        for (int k = 0; k < 4; k++) {
            std::vector<double> one(out_doubles(1, period, kWidths[k], R), -7.0), other(out_doubles(1, period, kWidths[(k + 1) % 4], R));
            double* d1[2] = {other.data(), one.data()};
            const uint64_t c2[2] = {comp[(k + 1) % 4], comp[k]};
            if (sixdof_history_quantiles(r.h, c2, 2, first + j * every, 1, 5, period, q.num.data(), q.den, R, d1, j % 2 ? SIXDOF_QUANTILE_ASYNC : 0u) != SIXDOF_OK ||
                sixdof_download_wait(r.h) != SIXDOF_OK)
                return complain(what + ": single-sample read: " + sixdof_last_error(r.h));
            if (std::memcmp(one.data(), &out[k][j * one.size()], one.size() * sizeof(double)) != 0)
                complain(what + ": " + kNames[k] + " sample " + std::to_string(j) + " of the range differs from the single-sample read of its tick");
        }
    if (sixdof_sync(r.h) != SIXDOF_OK) complain(what + ": sync");
}

// every order statistic of the crafted block: ranks k / (n - 1), k = 0 .. n - 1, sixteen at a time
template <class T>
void crafted_case(uint64_t n, uint32_t period) {
    Recorded<T> r(n, 4, 5, false, true);
    const uint64_t vel = sixdof_component_id("world_vel"), rows = n / period;
    for (uint64_t k0 = 0; k0 < rows; k0 += 16) {
        Ranks q{{}, static_cast<uint32_t>(rows - 1)};
        for (uint64_t k = k0; k < std::min(rows, k0 + 16); k++) q.num.push_back(static_cast<uint32_t>(k));
        std::vector<double> out(out_doubles(2, period, 6, q.num.size()), -7.0);
        double* dst[1] = {out.data()};
        if (sixdof_history_quantiles(r.h, &vel, 1, 4, 2, 1, period, q.num.data(), q.den, q.num.size(), dst, 0) != SIXDOF_OK) return complain(std::string("crafted: ") + sixdof_last_error(r.h));
        check_values(r, 1, 4, 2, 1, period, q, out, std::string(sizeof(T) == 4 ? "f32" : "f64") + " crafted, period " + std::to_string(period));
    }
}

void refusals() {
    Recorded<double> r(24, 6, 10, false);   // recording since tick 3, the ring keeps 5 .. 10
    const uint64_t pos = sixdof_component_id("world_pos"), inertia = sixdof_component_id("inertia");
    const uint32_t num[17] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16}, above[2] = {1, 21};
    std::vector<double> buf(out_doubles(4, 24, 7, 16), 123.0);
    double* dst[1] = {buf.data()};
    double* null_dst[1] = {nullptr};
    auto expect = [&](const char* what, int rc, int want) {
        if (rc != want) complain(std::string("refusal: ") + what + ": status " + std::to_string(rc) + ", expected " + std::to_string(want));
        else if (want != SIXDOF_OK && !*sixdof_last_error(r.h)) complain(std::string("refusal: ") + what + ": no message");
        for (double v : buf)
            if (v != 123.0) return complain(std::string("refusal: ") + what + ": something was copied"), void();
    };
    auto read = [&](const uint64_t* comp, uint64_t first, uint64_t samples, uint64_t every, uint32_t period, const uint32_t* nums, uint32_t den, size_t n_ranks,
                    double* const* to, uint32_t flags) { return sixdof_history_quantiles(r.h, comp, 1, first, samples, every, period, nums, den, n_ranks, to, flags); };
    expect("every = 0", read(&pos, 5, 2, 0, 1, num, 20, 2, dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("period = 0", read(&pos, 5, 2, 1, 0, num, 20, 2, dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("period does not divide n", read(&pos, 5, 2, 1, 7, num, 20, 2, dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("fallen out of the ring", read(&pos, 4, 2, 1, 1, num, 20, 2, dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("beyond tick", read(&pos, 9, 3, 1, 1, num, 20, 2, dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("last sample beyond tick", read(&pos, 5, 3, 3, 1, num, 20, 2, dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("unknown flags", read(&pos, 5, 2, 1, 1, num, 20, 2, dst, 2u), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("null buffer", read(&pos, 5, 2, 1, 1, num, 20, 2, null_dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("null buffer list", read(&pos, 5, 2, 1, 1, num, 20, 2, nullptr, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("no ranks", read(&pos, 5, 2, 1, 1, num, 20, 0, dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("17 ranks", read(&pos, 5, 2, 1, 1, num, 20, 17, dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("null ranks", read(&pos, 5, 2, 1, 1, nullptr, 20, 2, dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("denominator 0", read(&pos, 5, 2, 1, 1, num, 0, 2, dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("numerator above the denominator", read(&pos, 5, 2, 1, 1, above, 20, 2, dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    expect("inertia is not recorded", read(&inertia, 5, 2, 1, 1, num, 20, 2, dst, 0), SIXDOF_ERR_COMPONENT_NOT_FOUND);
    expect("no samples", read(&pos, 99, 0, 7, 1, num, 20, 2, dst, 0), SIXDOF_OK);
    if (read(&pos, 5, 4, 1, 24, num, 16, 16, dst, 0) != SIXDOF_OK || buf.back() == 123.0) complain("one row per group (period = n) with 16 ranks is refused or fills nothing");
    std::fill(buf.begin(), buf.end(), 123.0);
    if (sixdof_set_history(r.h, 0) != SIXDOF_OK) complain("refusal: set_history(0)");
    expect("no ring", read(&pos, 5, 2, 1, 1, num, 20, 2, dst, 0), SIXDOF_ERR_INVALID_ARGUMENT);
    // the width limit: 96 rows in groups of 96 are 576 bins of world_vel; 48 x 6 = 288 are served, with 16 ranks in several column ranges
    Recorded<double> wide(96, 4, 4, false);
    const uint64_t vel = sixdof_component_id("world_vel");
    std::vector<double> big(out_doubles(1, 96, 6, 16), 123.0);
    double* bdst[1] = {big.data()};
    int rc = sixdof_history_quantiles(wide.h, &vel, 1, 4, 1, 1, 96, num, 16, 16, bdst, 0);
    if (rc != SIXDOF_ERR_INVALID_ARGUMENT || !std::strstr(sixdof_last_error(wide.h), "512")) complain("refusal: period x width beyond the limit is not refused with the limit named");
    for (double v : big)
        if (v != 123.0) return complain("refusal: period x width beyond the limit: something was copied");
    if (sixdof_history_quantiles(wide.h, &vel, 1, 4, 1, 1, 48, num, 16, 16, bdst, 0) != SIXDOF_OK) complain(std::string("period 48 x width 6: ") + sixdof_last_error(wide.h));
    check_values(wide, 1, 4, 1, 1, 48, Ranks{std::vector<uint32_t>(num, num + 16), 16}, big, "period 48, 16 ranks");
}

// A range that one launch cannot cover: 65,538 samples of a one-row world.  The scratch budget of a launch cuts it first (a slot's
// histogram is 1 KiB, so 65,535 samples of the 6 or 7 slots of a Body column never fit one launch), the grid's 65,535 after it.
void long_range() {
    Recorded<double> r(1, 65540, 65540, false);
    const uint64_t comp[2] = {sixdof_component_id("world_pos"), sixdof_component_id("force")};
    const uint64_t n_samples = 65538;
    const Ranks q{{1, 0, 2}, 2};
    std::vector<double> out[2];
    double* dst[2];
    for (int k = 0; k < 2; k++) out[k].assign(out_doubles(n_samples, 1, k ? 6 : 7, 3), -7.0), dst[k] = out[k].data();
    if (sixdof_history_quantiles(r.h, comp, 2, 3, n_samples, 1, 1, q.num.data(), q.den, 3, dst, 0) != SIXDOF_OK) return complain(std::string("long range: ") + sixdof_last_error(r.h));
    check_values(r, 0, 3, n_samples, 1, 1, q, out[0], "long range");
    check_values(r, 3, 3, n_samples, 1, 1, q, out[1], "long range");
}

// Two staged readers pending on one copy lane: an asynchronous envelope read and an asynchronous quantile read behind it, then ONE
// sixdof_download_wait.  Both equal their blocking reads byte for byte, and sixdof_sync ends the page locks.
void two_readers_one_lane() {
    Recorded<double> r(24, 4, 6, false);
    const uint64_t comp[2] = {sixdof_component_id("world_pos"), sixdof_component_id("world_vel")};
    const Ranks q{{1, 50, 99}, 100};
    std::vector<double> env[2][2], qu[2][2];
    for (int blocking = 0; blocking < 2; blocking++) {
        double *e[2], *d[2];
        for (int k = 0; k < 2; k++) {
            env[blocking][k].assign(3 * 2 * 5 * kWidths[k], -7.0), qu[blocking][k].assign(out_doubles(3, 2, kWidths[k], 3), -7.0);
            e[k] = env[blocking][k].data(), d[k] = qu[blocking][k].data();
        }
        if (sixdof_history_envelope(r.h, comp, 2, 4, 3, 1, 2, e, blocking ? 0u : SIXDOF_ENVELOPE_ASYNC) != SIXDOF_OK ||
            sixdof_history_quantiles(r.h, comp, 2, 4, 3, 1, 2, q.num.data(), q.den, 3, d, blocking ? 0u : SIXDOF_QUANTILE_ASYNC) != SIXDOF_OK)
            return complain(std::string("two readers on one lane: ") + sixdof_last_error(r.h));
        if (!blocking && (sixdof_download_wait(r.h) != SIXDOF_OK || sixdof_sync(r.h) != SIXDOF_OK)) complain("two readers on one lane: download_wait / sync");
        if (!blocking && hip_fake::live_page_locks()) complain("two readers on one lane: page locks are alive after sixdof_sync");
    }
    for (int k = 0; k < 2; k++) {
        if (env[0][k] != env[1][k] && std::memcmp(env[0][k].data(), env[1][k].data(), env[0][k].size() * 8) != 0) complain("two readers on one lane: the envelope differs from its blocking read");
        if (std::memcmp(qu[0][k].data(), qu[1][k].data(), qu[0][k].size() * 8) != 0) complain("two readers on one lane: the quantiles differ from their blocking read");
        check_values(r, k, 4, 3, 1, 2, q, qu[0][k], "two readers on one lane");
    }
}

// Each fallible runtime call of a blocking and of an asynchronous read is failed once: the status is returned with a message,
// the call succeeds when repeated, its values are the fault-free run's, the ring is intact, and nothing outlives the handle.
void failure_injection() {
    const uint64_t comp[2] = {sixdof_component_id("world_pos"), sixdof_component_id("force")};
    const Ranks q{{1, 25, 50, 75, 99}, 100};
    std::vector<double> want[2];
    long n_calls = 0;
    for (long fault = -1; fault < n_calls || fault < 0; fault++) {
        const std::string run = "fault at call " + std::to_string(fault);
        {
            Recorded<double> r(40, 8, 9, true);
            std::vector<double> out[2][2];
            int failed = 0;
            const long calls0 = hip_fake::calls();
            hip_fake::fail_after(fault);
            for (int a = 0; a < 2; a++) {   // blocking, then asynchronous: the second grows neither buffer
                double* dst[2];
                for (int k = 0; k < 2; k++) out[a][k].assign(out_doubles(3, 4, k ? 6 : 7, 5), -1.0), dst[k] = out[a][k].data();
                auto read = [&] { return sixdof_history_quantiles(r.h, comp, 2, 4, 3, 2, 4, q.num.data(), q.den, 5, dst, a ? SIXDOF_QUANTILE_ASYNC : 0u); };
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
                check_values(r, 0, 4, 3, 2, 4, q, want[0], "fault-free run");
                check_values(r, 3, 4, 3, 2, 4, q, want[1], "fault-free run");
            } else if (failed != 1) {
                complain(run + ": " + std::to_string(failed) + " steps reported it");
            }
            for (int a = 0; a < 2; a++)
                for (int k = 0; k < 2; k++)
                    if (std::memcmp(out[a][k].data(), want[k].data(), want[k].size() * sizeof(double)) != 0) complain(run + ": the values after the retry differ from the fault-free run's");
            // the ring is intact: tick 9 of world_pos is what was uploaded before it
            std::vector<double> block(40 * 7);
            if (sixdof_history_read(r.h, comp[0], 9, block.data()) != SIXDOF_OK || std::memcmp(block.data(), r.truth[0][8].data(), block.size() * 8) != 0)
                complain(run + ": the ring is not what it was");
        }
        if (hip_fake::live_allocations() || hip_fake::live_streams() || hip_fake::live_events() || hip_fake::live_page_locks()) complain(run + ": something outlives sixdof_destroy");
    }
    std::printf("quantile_host_test: %ld fallible calls of a blocking and an asynchronous read, each failed once\n", n_calls);
}

}  // namespace

int main() {
    const Ranks usual{{0, 1, 50, 99, 100, 50}, 100}, one{{1}, 2}, many{{0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, 15};
    values_case<double>(300, 10, 27, 18, 3, 1, true, usual);      // the range wraps the ring; diverged rows, an all-NaN element
    values_case<double>(4099, 4, 5, 3, 2, 1, false, usual);       // several row blocks, a ragged last sweep; top bytes shared on world_pos
    values_case<double>(300, 8, 9, 9, 1, 12, true, usual);        // groups: 84 bins of world_pos in column ranges of 8
    values_case<double>(320, 4, 5, 4, 1, 64, false, one);         // 448 bins of world_pos, one rank
    values_case<double>(300, 4, 5, 5, 1, 1, true, many);          // 16 ranks: the 7 bins of world_pos in column ranges of 3
    values_case<float>(64, 8, 8, 3, 1, 1, true, usual);
    values_case<double>(1, 4, 4, 4, 1, 1, false, usual);
    values_case<double>(65, 4, 4, 3, 1, 5, false, usual);
    crafted_case<double>(300, 1);
    crafted_case<float>(300, 1);
    crafted_case<double>(300, 3);
    refusals();
    two_readers_one_lane();
    long_range();
    failure_injection();
    if (hip_fake::violations()) complain(std::to_string(hip_fake::violations()) + " violations reported by the fake runtime");
    if (g_failures) return std::fprintf(stderr, "quantile_host_test: %d failures\n", g_failures), 1;
    std::printf("quantile_host_test: ok\n");
    return 0;
}
