// quantile_host_test.cpp — sixdof_history_quantiles (sixdof_capi.cpp) over the fake runtime (hip_fake.cpp), whose launcher selects
// through quantile_plan.hpp's keys, scan step and lo -> hi rule, under AddressSanitizer / UBSan, no GPU: `make quantile_test`,
// tests/test_history_quantiles_host.py.
//
// The ring (force with many ties) and the cases every reduction shares are ring_host_fixture.hpp's.  Checked: every value bitwise
// against std::sort on the keys, over random and crafted blocks (ties, runs, values apart in the lowest byte only or in sign and
// exponent only, +-0, denormals, +-max, NaN, +-inf), every refusal with nothing copied, bit-identity of a range's samples with
// single-sample reads, more components than one launch covers, a range long enough to be cut into several launches, and every
// fallible runtime call of the entry point failed once.
#include <algorithm>

#include "ring_host_fixture.hpp"

namespace {

using sixdof::QuantileBits;

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
    Recorded<T> r(n, ring, ticks, {holes, craft, true});
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
    Recorded<T> r(n, 4, 5, {false, true, true});
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

// the entry point with these ranks bound
RingRead with_ranks(const uint32_t* num, uint32_t den, size_t n_ranks) {
    return [=](sixdof_handle* h, const uint64_t* comp, size_t n_comp, uint64_t first, uint64_t samples, uint64_t every, uint32_t period, double* const* dst,
               uint32_t flags) { return sixdof_history_quantiles(h, comp, n_comp, first, samples, every, period, num, den, n_ranks, dst, flags); };
}
const uint32_t kNum[17] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};

// the common table with 2 ranks over 20, the reads it serves with 16 over 16 (48 x 6 bins then go in several column ranges); the rank checks
void refusals() {
    refusal_table(
        1 + 2 * 16, with_ranks(kNum, 20, 2), with_ranks(kNum, 16, 16),
        [](sixdof_handle* h, const uint64_t* pos, double* const* dst, const Expect& expect) {
            static const uint32_t above[2] = {1, 21};
            auto read = [&](const uint32_t* nums, uint32_t den, size_t n_ranks) { return with_ranks(nums, den, n_ranks)(h, pos, 1, 5, 2, 1, 1, dst, 0); };
            expect("no ranks", read(kNum, 20, 0), SIXDOF_ERR_INVALID_ARGUMENT);
            expect("17 ranks", read(kNum, 20, 17), SIXDOF_ERR_INVALID_ARGUMENT);
            expect("null ranks", read(nullptr, 20, 2), SIXDOF_ERR_INVALID_ARGUMENT);
            expect("denominator 0", read(kNum, 0, 2), SIXDOF_ERR_INVALID_ARGUMENT);
            expect("numerator above the denominator", read(above, 20, 2), SIXDOF_ERR_INVALID_ARGUMENT);
        },
        [](const Recorded<double>& wide, const std::vector<double>& big) {
            check_values(wide, 1, 4, 1, 1, 48, Ranks{std::vector<uint32_t>(kNum, kNum + 16), 16}, big, "period 48, 16 ranks");
        });
}

// A range that one launch cannot cover: 65,538 samples of a one-row world.  The scratch budget of a launch cuts it first (a slot's
// histogram is 1 KiB, so 65,535 samples of the 6 or 7 slots of a Body column never fit one launch), the grid's 65,535 after it.
void long_range() {
    Recorded<double> r(1, 65540, 65540, {false, false, true});
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
    Recorded<double> r(24, 4, 6, {false, false, true});
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

// What the fault sweep reads: ticks 4, 6, 8 of world_pos and force, five ranks in four groups.  After every run the ring is intact,
// and the fault-free values are the sorted ones.
const Ranks kSweptRanks{{1, 25, 50, 75, 99}, 100};
const SweptRead kSwept{
    "quantile", {}, [](int k) { return out_doubles(3, 4, k ? 6 : 7, 5); },
    [](sixdof_handle* h, const uint64_t* comp, void* const dst[2], bool async) {
        return with_ranks(kSweptRanks.num.data(), kSweptRanks.den, 5)(h, comp, 2, 4, 3, 2, 4, reinterpret_cast<double* const*>(dst), async ? SIXDOF_QUANTILE_ASYNC : 0u);
    },
    [](const Recorded<double>& r, bool fault_free, const std::vector<double> want[2], const std::string& run) {
        if (fault_free) {
            check_values(r, 0, 4, 3, 2, 4, kSweptRanks, want[0], "fault-free run");
            check_values(r, 3, 4, 3, 2, 4, kSweptRanks, want[1], "fault-free run");
        }
        std::vector<double> block(40 * 7);   // tick 9 of world_pos is what was uploaded before it
        if (sixdof_history_read(r.h, sixdof_component_id("world_pos"), 9, block.data()) != SIXDOF_OK || std::memcmp(block.data(), r.truth[0][8].data(), block.size() * 8) != 0)
            complain(run + ": the ring is not what it was");
    }};

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
    more_components_than_one_launch_covers(1 + 2 * usual.num.size(), with_ranks(usual.num.data(), usual.den, usual.num.size()), {false, false, true});
    two_readers_one_lane();
    long_range();
    failure_injection("quantile_host_test", kSwept, {true, false, true});
    failure_injection("quantile_host_test", kSwept, {true, false, true}, hip_fake::kCopyFirst);
    return verdict("quantile_host_test");
}
