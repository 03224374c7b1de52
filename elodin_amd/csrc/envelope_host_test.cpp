// envelope_host_test.cpp — sixdof_history_envelope (sixdof_capi.cpp) over the fake runtime (hip_fake.cpp), whose launcher computes
// the real reduction through envelope_plan.hpp in the kernels' geometry and merge order, under AddressSanitizer / UBSan, no GPU:
// `make envelope_test`, tests/test_history_envelope_host.py.
//
// The ring and the cases every reduction shares are ring_host_fixture.hpp's.  Checked: the values against a long-double
// two-pass reference, every refusal with nothing copied, bit-identity of a range's samples with single-sample reads, more
// components than one launch covers, and every fallible runtime call of the entry point failed once.  The readers that share
// its copy lane and staging rules ride along: sixdof_watch_read in the same fault sweep, both pending on one lane,
// sixdof_history_stream across the ring's wrap.
#include "ring_host_fixture.hpp"

namespace {

size_t out_doubles(uint64_t n_samples, uint32_t period, uint64_t w) { return n_samples * period * sixdof::kEnvelopeStats * w; }

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
    Recorded<T> r(n, ring, ticks, {holes});
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

const RingRead kEnvelope = [](sixdof_handle* h, const uint64_t* comp, size_t n_comp, uint64_t first, uint64_t samples, uint64_t every, uint32_t period,
                               double* const* dst, uint32_t flags) { return sixdof_history_envelope(h, comp, n_comp, first, samples, every, period, dst, flags); };

// Two staged readers pending on one copy lane: an asynchronous watch read, an asynchronous envelope read behind it and — with
// `regrow` — a second, larger watch read whose staging buffer has to grow while the first two are pending, then ONE
// sixdof_download_wait.  Everything equals the blocking reads of the same ranges byte for byte, and sixdof_sync ends the page locks.
void two_readers_one_lane(bool regrow) {
    const std::string what = regrow ? "two readers, staging regrown while pending" : "two readers on one lane";
    Recorded<double> r(24, 4, 6);   // recording since tick 3: the ring of 4 holds 3 .. 6, tick 5 in slot 0
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
    Recorded<double> r(24, 4, 6);
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
const uint64_t kSweptEntities[3] = {1, 17, 40};
const auto kFilled = [](const Recorded<double>&, bool fault_free, const std::vector<double> want[2], const std::string& run) {
    if (fault_free && (want[0][0] == -1.0 || want[1].back() == -1.0)) complain(run + ": the fault-free read filled nothing");
};
const SweptRead kSweptReads[2] = {
    {"envelope", {}, [](int k) { return out_doubles(3, 4, k ? 6 : 7); },
     [](sixdof_handle* h, const uint64_t* comp, void* const dst[2], bool async) {
         return sixdof_history_envelope(h, comp, 2, 4, 3, 2, 4, reinterpret_cast<double* const*>(dst), async ? SIXDOF_ENVELOPE_ASYNC : 0u);
     }, kFilled},
    {"watch", [](sixdof_handle* h, const uint64_t* comp) { return sixdof_set_watch(h, comp, 2, kSweptEntities, 3); }, [](int k) { return size_t(3 * 3 * (k ? 6 : 7)); },
     [](sixdof_handle* h, const uint64_t*, void* const dst[2], bool async) { return sixdof_watch_read(h, 4, 3, 2, dst, async ? SIXDOF_WATCH_ASYNC : 0u); }, kFilled},
};

}  // namespace

int main() {
    values_case<double>(300, 10, 27, 18, 3, 1, true);     // the range wraps the ring; diverged rows
    values_case<double>(4099, 4, 5, 3, 2, 1, false);      // several blocks, a ragged last tile; the conditioning case on world_pos
    values_case<double>(300, 8, 9, 9, 1, 12, true);       // groups
    values_case<double>(320, 4, 5, 4, 1, 64, false);      // a wavefront-sized world: 448 bins of world_pos
    values_case<float>(64, 8, 8, 3, 1, 1, true);
    values_case<double>(1, 4, 4, 4, 1, 1, false);
    values_case<double>(65, 4, 4, 3, 1, 5, false);
    refusal_table(sixdof::kEnvelopeStats, kEnvelope, kEnvelope);
    more_components_than_one_launch_covers(sixdof::kEnvelopeStats, kEnvelope);
    two_readers_one_lane(false);
    two_readers_one_lane(true);
    stream_across_the_wrap();
    for (const SweptRead& swept : kSweptReads) failure_injection("envelope_host_test", swept, {true});
    for (const SweptRead& swept : kSweptReads) failure_injection("envelope_host_test", swept, {true}, hip_fake::kCopyFirst);
    return verdict("envelope_host_test");
}
