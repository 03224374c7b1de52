// covariance_host_test.cpp — sixdof_history_covariance (sixdof_capi.cpp) over the fake runtime (hip_fake.cpp), whose launcher
// reduces through covariance_plan.hpp in the kernels' geometry and merge order, under AddressSanitizer / UBSan and without FMA
// contraction, no GPU: `make covariance_test`, tests/test_history_covariance_host.py.
//
// Checked: update and merge against a long-double two-pass reference under the bounds the GPU tests use; merging with the empty
// record and a channel listed twice; the entry point against a serial walk of the plan's geometry, bit for bit, over row counts,
// periods, channel counts and both dtypes; forced small sample chunks; every refusal with nothing copied; every fallible runtime
// call of the entry point failed once.  The ring is ring_host_fixture.hpp's.
#include <algorithm>
#include <set>

#include "covariance_plan.hpp"
#include "ring_host_fixture.hpp"

namespace {

using namespace sixdof;

// the device limit, per instantiation: the records of a stage-1 block in the LDS of a CU
static_assert(covariance_lds_bytes(2) <= 160 * 1024 && covariance_lds_bytes(3) <= 160 * 1024 && covariance_lds_bytes(4) <= 160 * 1024 &&
                  covariance_lds_bytes(5) <= 160 * 1024 && covariance_lds_bytes(6) <= 160 * 1024,
              "LDS of a stage-1 block");
static_assert(kCovarianceMaxChannels == SIXDOF_COVARIANCE_MAX_CHANNELS, "the plan and the header disagree about the channel limit");

const double kEps = std::numeric_limits<double>::epsilon();

struct Channel { int comp; uint32_t element; };   // comp: index into kNames
std::vector<sixdof_cov_channel> abi(const std::vector<Channel>& ch) {
    std::vector<sixdof_cov_channel> v;
    for (const Channel& c : ch) v.push_back(sixdof_cov_channel{sixdof_component_id(kNames[c.comp]), c.element, 0});
    return v;
}
const std::vector<Channel> kLists[4] = {
    {{1, 0}, {1, 1}},                                       // inside one component
    {{0, 4}, {0, 5}, {1, 3}},
    {{0, 4}, {0, 5}, {0, 6}, {1, 3}, {3, 2}},               // three components
    {{0, 4}, {0, 5}, {0, 6}, {1, 3}, {1, 4}, {1, 5}},       // position and velocity
};

// ---- the arithmetic ------------------------------------------------------------------------------------------------------
// `rows` rows of K values: the records of two halves, updated row by row and merged, against the two-pass reference.
template <int K>
void arithmetic_case(const char* what, const std::vector<double>& x, double* worst_mean, double* worst_c) {
    const size_t rows = x.size() / K;
    for (size_t cut : {size_t(0), rows / 3, rows / 2, rows}) {
        CovarianceRecord<K> left = covariance_empty<K>(), right = covariance_empty<K>();
        for (size_t r = 0; r < rows; r++) {
            double v[K];
            for (int a = 0; a < K; a++) v[a] = x[r * K + a];
            covariance_accumulate<K>(r < cut ? left : right, v);
        }
        const CovarianceRecord<K> got = covariance_merge<K>(left, right);
        long double mean[K], m2[K], sq[K], abs_sum[K];
        double c = 0;
        std::vector<size_t> used;
        for (size_t r = 0; r < rows; r++) {
            bool ok = true;
            for (int a = 0; a < K; a++) ok = ok && std::isfinite(x[r * K + a]);
            if (ok) used.push_back(r);
        }
        c = static_cast<double>(used.size());
        if (got.count != c) { complain(std::string(what) + ": count"); continue; }
        if (c == 0) continue;
        for (int a = 0; a < K; a++) {
            mean[a] = m2[a] = sq[a] = abs_sum[a] = 0;
            for (size_t r : used) mean[a] += x[r * K + a], sq[a] += static_cast<long double>(x[r * K + a]) * x[r * K + a], abs_sum[a] += std::fabs(x[r * K + a]);
            mean[a] /= c;
            for (size_t r : used) m2[a] += (x[r * K + a] - mean[a]) * (x[r * K + a] - mean[a]);
        }
        for (int a = 0; a < K; a++) {
            const double bound = 2 * c * kEps * static_cast<double>(abs_sum[a] / c), err = std::fabs(static_cast<double>(got.mean[a] - mean[a]));
            if (bound > 0) *worst_mean = std::max(*worst_mean, err / bound);
            if (!(err <= bound)) complain(std::string(what) + ": mean off by " + std::to_string(err) + ", bound " + std::to_string(bound));
            for (int b = a; b < K; b++) {
                long double ref = 0;
                for (size_t r : used) ref += (x[r * K + a] - mean[a]) * (x[r * K + b] - mean[b]);
                const double cb = c * kEps * (std::sqrt(static_cast<double>(m2[a] * sq[b])) + std::sqrt(static_cast<double>(m2[b] * sq[a])));
                const double ce = std::fabs(static_cast<double>(got.c[covariance_pair(K, a, b)] - ref));
                if (cb > 0) *worst_c = std::max(*worst_c, ce / cb);
                if (!(ce <= cb)) complain(std::string(what) + ": C[" + std::to_string(a) + "][" + std::to_string(b) + "] off by " + std::to_string(ce) + ", bound " + std::to_string(cb));
            }
        }
    }
}
void arithmetic() {
    std::mt19937_64 rng(7);
    std::normal_distribution<double> normal(0.0, 1.0);
    double worst_mean = 0, worst_c = 0;
    for (size_t rows : {size_t(2), size_t(3), size_t(17), size_t(300), size_t(5000)}) {
        std::vector<double> orbit(rows * 3), mixed(rows * 6), anti(rows * 2), drift(rows * 2), holes(rows * 3);
        for (size_t r = 0; r < rows; r++) {
            for (int a = 0; a < 3; a++) orbit[r * 3 + a] = 6.4e6 + normal(rng);                                   // 6.4e6 m, metre spreads
            for (int a = 0; a < 6; a++) mixed[r * 6 + a] = (a % 2 ? 7e6 : -3.0) + std::pow(10.0, a - 3) * normal(rng);   // scales 1e-3 .. 1e2, offsets to 7e6
            const double z = normal(rng);
            anti[r * 2] = 100.0 + z, anti[r * 2 + 1] = 100.0 - z + 1e-9 * normal(rng);                            // near-perfect anti-correlation
            drift[r * 2] = 1e3 + 0.5 * double(r) + normal(rng), drift[r * 2 + 1] = -2.0 * double(r) + normal(rng);     // drifting rows
            for (int a = 0; a < 3; a++) holes[r * 3 + a] = normal(rng);
            if (r % 5 == 1) holes[r * 3 + r % 3] = r % 2 ? NAN : INFINITY;
        }
        arithmetic_case<3>("orbit", orbit, &worst_mean, &worst_c);
        arithmetic_case<6>("mixed scales", mixed, &worst_mean, &worst_c);
        arithmetic_case<2>("anti-correlated", anti, &worst_mean, &worst_c);
        arithmetic_case<2>("drift", drift, &worst_mean, &worst_c);
        arithmetic_case<3>("holes", holes, &worst_mean, &worst_c);
    }
    std::printf("arithmetic: worst error / bound: mean %.4f, co-moment %.4f\n", worst_mean, worst_c);
}

void merge_properties() {
    std::mt19937_64 rng(11);
    std::normal_distribution<double> normal(5.0, 2.0);
    CovarianceRecord<3> r = covariance_empty<3>(), twice = covariance_empty<3>(), other = covariance_empty<3>();
    for (int i = 0; i < 40; i++) {
        const double u = normal(rng), v = normal(rng);
        const double x[3] = {u, v, u};   // channel 0 listed again as channel 2
        covariance_accumulate<3>(i < 25 ? twice : other, x);
        covariance_accumulate<3>(r, x);
    }
    const CovarianceRecord<3> empty = covariance_empty<3>();
    const CovarianceRecord<3> a = covariance_merge<3>(r, empty), b = covariance_merge<3>(empty, r);
    if (std::memcmp(&a, &r, sizeof r) != 0 || std::memcmp(&b, &r, sizeof r) != 0) complain("merge with the empty record is not the identity");
    const CovarianceRecord<3> e2 = covariance_merge<3>(empty, empty);
    if (e2.count != 0.0) complain("two empty records do not merge into one");
    for (const CovarianceRecord<3>& m : {r, covariance_merge<3>(twice, other)}) {
        const double aa = m.c[covariance_pair(3, 0, 0)], ab = m.c[covariance_pair(3, 0, 2)], bb = m.c[covariance_pair(3, 2, 2)];
        if (std::memcmp(&aa, &ab, 8) != 0 || std::memcmp(&aa, &bb, 8) != 0 || std::memcmp(&m.mean[0], &m.mean[2], 8) != 0)
            complain("a channel listed twice: C_aa, C_ab, C_bb are not bit-equal");
    }
}

// ---- the entry point against a serial walk of the plan -----------------------------------------------------------------------
template <class T, int K>
void walk_tick(const Recorded<T>& r, const std::vector<Channel>& ch, uint64_t tick, uint32_t period, double* to) {
    const CovarianceGeom g = covariance_geom(r.n, period);
    std::vector<CovarianceRecord<K>> block(size_t(g.blocks) * period), rec(kCovarianceThreads);
    for (uint32_t b = 0; b < g.blocks; b++) {
        for (uint32_t t = 0; t < g.tile; t++) {
            rec[t] = covariance_empty<K>();
            for (uint64_t row = uint64_t(b) * g.tile + t; row < r.n; row += uint64_t(g.blocks) * g.tile) {
                double x[K];
                for (int a = 0; a < K; a++) x[a] = static_cast<double>(r.truth[ch[a].comp][tick - 1][row * kWidths[ch[a].comp] + ch[a].element]);
                covariance_accumulate<K>(rec[t], x);
            }
        }
        for (uint32_t grp = 0; grp < period; grp++) {
            covariance_tree_fold<K>(&rec[grp], g.per_group, period);
            block[size_t(b) * period + grp] = rec[grp];
        }
    }
    for (uint32_t grp = 0; grp < period; grp++) {
        CovarianceRecord<K> m = block[grp];
        for (uint32_t b = 1; b < g.blocks; b++) m = covariance_merge<K>(m, block[size_t(b) * period + grp]);
        covariance_emit<K>(m, to + size_t(grp) * covariance_fields(K));
    }
}
template <class T>
void walk(const Recorded<T>& r, const std::vector<Channel>& ch, uint64_t tick, uint32_t period, double* to) {
    switch (ch.size()) {
    case 2: return walk_tick<T, 2>(r, ch, tick, period, to);
    case 3: return walk_tick<T, 3>(r, ch, tick, period, to);
    case 4: return walk_tick<T, 4>(r, ch, tick, period, to);
    case 5: return walk_tick<T, 5>(r, ch, tick, period, to);
    default: return walk_tick<T, 6>(r, ch, tick, period, to);
    }
}

template <class T>
void bit_identity_case(uint64_t n_listed, uint32_t period) {
    const uint64_t n = (n_listed + period - 1) / period * period;   // the listed row count, or the next multiple of the period
    Recorded<T> r(n, 4, 5, {n > 3});                                // recording since tick 3: samples 3, 4, 5; diverged world_vel rows
    for (const std::vector<Channel>& ch : kLists) {
        const size_t F = covariance_fields(static_cast<uint32_t>(ch.size()));
        const std::string what = std::string(sizeof(T) == 4 ? "f32" : "f64") + " n " + std::to_string(n) + " period " + std::to_string(period) + " k " + std::to_string(ch.size());
        const std::vector<sixdof_cov_channel> c = abi(ch);
        std::vector<double> got(3 * period * F, -7.0), want(3 * period * F, -9.0), one(period * F, -7.0);
        if (sixdof_history_covariance(r.h, c.data(), c.size(), 3, 3, 1, period, got.data(), 0) != SIXDOF_OK) return complain(what + ": " + sixdof_last_error(r.h));
        for (uint64_t j = 0; j < 3; j++) walk(r, ch, 3 + j, period, &want[j * period * F]);
        if (!same_bits(got, want)) complain(what + ": the read differs from the serial walk of the plan");
        // the middle tick alone, asynchronously, with another `every`
        if (sixdof_history_covariance(r.h, c.data(), c.size(), 4, 1, 9, period, one.data(), SIXDOF_COVARIANCE_ASYNC) != SIXDOF_OK || sixdof_download_wait(r.h) != SIXDOF_OK)
            return complain(what + ": single-sample read: " + sixdof_last_error(r.h));
        if (std::memcmp(one.data(), &got[period * F], one.size() * sizeof(double)) != 0) complain(what + ": a tick read alone differs from the tick in its range");
        // listwise skipping shows in the counts: the world_vel holes are rows 0, n / 2, n - 1 (all elements) and row 1 element 2
        if (n > 3 && period == 1) {
            bool vel = false;
            for (const Channel& x : ch) vel = vel || x.comp == 1;
            std::set<uint64_t> dropped = {0, n / 2, n - 1};
            for (const Channel& x : ch)
                if (x.comp == 1 && x.element == 2) dropped.insert(1);
            const double expect = vel ? double(n - dropped.size()) : double(n);
            if (got[0] != expect) complain(what + ": count " + std::to_string(got[0]) + ", expected " + std::to_string(expect));
        }
    }
    if (sixdof_sync(r.h) != SIXDOF_OK) complain("sync");
}

void chunking() {
    Recorded<double> r(300, 10, 12, {true});   // the ring keeps 3 .. 12
    const std::vector<sixdof_cov_channel> c = abi(kLists[3]);
    const size_t F = covariance_fields(6);
    std::vector<double> whole(8 * 4 * F, -7.0);
    force_segments("SIXDOF_COVARIANCE_CHUNK", 0);
    if (sixdof_history_covariance(r.h, c.data(), 6, 4, 8, 1, 4, whole.data(), 0) != SIXDOF_OK) return complain(std::string("chunking: ") + sixdof_last_error(r.h));
    for (uint64_t chunk : {1, 3, 5, 8, 100}) {
        force_segments("SIXDOF_COVARIANCE_CHUNK", chunk);
        std::vector<double> cut(whole.size(), -9.0);
        if (sixdof_history_covariance(r.h, c.data(), 6, 4, 8, 1, 4, cut.data(), chunk % 2 ? SIXDOF_COVARIANCE_ASYNC : 0u) != SIXDOF_OK || sixdof_download_wait(r.h) != SIXDOF_OK)
            complain(std::string("chunking: ") + sixdof_last_error(r.h));
        if (!same_bits(cut, whole)) complain("chunks of " + std::to_string(chunk) + " samples give other bits than one launch");
    }
    force_segments("SIXDOF_COVARIANCE_CHUNK", 0);
    if (sixdof_sync(r.h) != SIXDOF_OK) complain("chunking: sync");
}

// every sample of one (sample, group) entry of an all-non-finite group: count 0, the rest NaN
void empty_group() {
    Recorded<double> r(24, 4, 4, {true});   // force element 4 is NaN in every row
    const std::vector<sixdof_cov_channel> c = abi({{3, 4}, {0, 4}});
    std::vector<double> out(2 * covariance_fields(2), -7.0);
    if (sixdof_history_covariance(r.h, c.data(), 2, 4, 1, 1, 2, out.data(), 0) != SIXDOF_OK) return complain(std::string("empty group: ") + sixdof_last_error(r.h));
    for (size_t i = 0; i < out.size(); i++)
        if (i % covariance_fields(2) == 0 ? out[i] != 0.0 : !std::isnan(out[i])) complain("empty group: entry " + std::to_string(i) + " is " + std::to_string(out[i]));
}

void refusals() {
    Recorded<double> r(24, 6, 10);   // recording since tick 3, the ring keeps 5 .. 10
    std::vector<double> buf(4 * 24 * covariance_fields(6), 123.0);
    const std::vector<sixdof_cov_channel> six = abi(kLists[3]);
    std::vector<sixdof_cov_channel> seven = six, wide = six, reserved = six, unknown = six;
    seven.push_back(six[0]);
    wide[1].element = 7, reserved[2].reserved = 1, unknown[3].component_id = sixdof_component_id("inertia");
    auto expect = [&](const char* what, int rc, int want) {
        if (rc != want) complain(std::string("refusal: ") + what + ": status " + std::to_string(rc) + ", expected " + std::to_string(want));
        else if (want != SIXDOF_OK && !*sixdof_last_error(r.h)) complain(std::string("refusal: ") + what + ": no message");
        if (want != SIXDOF_OK) std::printf("refusal: %s: %s\n", what, sixdof_last_error(r.h));
        for (double v : buf)
            if (v != 123.0) return complain(std::string("refusal: ") + what + ": something was copied"), void();
    };
    auto read = [&](const std::vector<sixdof_cov_channel>& c, size_t k, uint64_t first, uint64_t samples, uint64_t every, uint32_t period, double* dst, uint32_t flags) {
        return sixdof_history_covariance(r.h, c.data(), k, first, samples, every, period, dst, flags);
    };
    const int bad = SIXDOF_ERR_INVALID_ARGUMENT;
    expect("every = 0", read(six, 6, 5, 2, 0, 1, buf.data(), 0), bad);
    expect("period = 0", read(six, 6, 5, 2, 1, 0, buf.data(), 0), bad);
    expect("period does not divide n", read(six, 6, 5, 2, 1, 7, buf.data(), 0), bad);
    expect("no channel", read(six, 0, 5, 2, 1, 1, buf.data(), 0), bad);
    expect("one channel", read(six, 1, 5, 2, 1, 1, buf.data(), 0), bad);
    if (!std::strstr(sixdof_last_error(r.h), "envelope")) complain("refusal: one channel: the message does not name the envelope");
    expect("seven channels", read(seven, 7, 5, 2, 1, 1, buf.data(), 0), bad);
    expect("null channels", sixdof_history_covariance(r.h, nullptr, 6, 5, 2, 1, 1, buf.data(), 0), bad);
    expect("null buffer", read(six, 6, 5, 2, 1, 1, nullptr, 0), bad);
    expect("element beyond the width", read(wide, 6, 5, 2, 1, 1, buf.data(), 0), bad);
    expect("reserved != 0", read(reserved, 6, 5, 2, 1, 1, buf.data(), 0), bad);
    expect("fallen out of the ring", read(six, 6, 4, 2, 1, 1, buf.data(), 0), bad);
    expect("beyond tick", read(six, 6, 9, 3, 1, 1, buf.data(), 0), bad);
    expect("last sample beyond tick", read(six, 6, 5, 3, 3, 1, buf.data(), 0), bad);
    expect("unknown flags", read(six, 6, 5, 2, 1, 1, buf.data(), 2u), bad);
    expect("inertia is not recorded", read(unknown, 6, 5, 2, 1, 1, buf.data(), 0), SIXDOF_ERR_COMPONENT_NOT_FOUND);
    expect("no samples", read(six, 6, 99, 0, 7, 1, buf.data(), 0), SIXDOF_OK);
    if (read(six, 6, 5, 4, 1, 24, buf.data(), 0) != SIXDOF_OK || buf.back() == 123.0) complain("one row per group (period = n) is refused or fills nothing");
    std::fill(buf.begin(), buf.end(), 123.0);
    if (sixdof_set_history(r.h, 0) != SIXDOF_OK) complain("refusal: set_history(0)");
    expect("no ring", read(six, 6, 5, 2, 1, 1, buf.data(), 0), bad);
    // the period limit: 514 rows in groups of 257 are refused with the limit named, 512 rows in groups of 256 are served
    Recorded<double> over(514, 4, 4), at(512, 4, 4);
    std::vector<double> big(257 * covariance_fields(6), 123.0);
    const int rc = sixdof_history_covariance(over.h, six.data(), 6, 4, 1, 1, 257, big.data(), 0);
    if (rc != bad || !std::strstr(sixdof_last_error(over.h), std::to_string(kCovarianceMaxPeriod).c_str())) complain("refusal: a period beyond the limit is not refused with the limit named");
    std::printf("refusal: %s: %s\n", "period beyond the limit", sixdof_last_error(over.h));
    for (double v : big)
        if (v != 123.0) return complain("refusal: period beyond the limit: something was copied");
    if (sixdof_history_covariance(at.h, six.data(), 6, 4, 1, 1, kCovarianceMaxPeriod, big.data(), 0) != SIXDOF_OK) complain(std::string("period at the limit: ") + sixdof_last_error(at.h));
}

// What the fault sweep reads: ticks 4, 6, 8 of five channels of world_pos and force in four groups (buffer 1 is not used).
const SweptRead kSwept = {
    "covariance", {}, [](int k) { return k ? size_t(1) : size_t(3 * 4 * covariance_fields(5)); },
    [](sixdof_handle* h, const uint64_t* comp, void* const dst[2], bool async) {
        const sixdof_cov_channel c[5] = {{comp[0], 4, 0}, {comp[1], 0, 0}, {comp[0], 5, 0}, {comp[1], 1, 0}, {comp[0], 4, 0}};
        return sixdof_history_covariance(h, c, 5, 4, 3, 2, 4, static_cast<double*>(dst[0]), async ? SIXDOF_COVARIANCE_ASYNC : 0u);
    },
    [](const Recorded<double>&, bool fault_free, const std::vector<double> want[2], const std::string& run) {
        if (fault_free && (want[0][0] == -1.0 || want[0].back() == -1.0)) complain(run + ": the fault-free read filled nothing");
    }};

}  // namespace

int main() {
    arithmetic();
    merge_properties();
    for (uint64_t n : {1, 2, 63, 64, 65, 300, 4099})
        for (uint32_t period : {1u, 4u, 12u, kCovarianceMaxPeriod}) {
            bit_identity_case<double>(n, period);
            bit_identity_case<float>(n, period);
        }
    chunking();
    empty_group();
    refusals();
    failure_injection("covariance_host_test", kSwept, {true});
    failure_injection("covariance_host_test", kSwept, {true}, hip_fake::kCopyFirst);
    return verdict("covariance_host_test");
}
