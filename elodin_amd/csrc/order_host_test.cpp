// order_host_test.cpp — the host layer's stream order, buffer lifetimes and page-lock extents (sixdof_capi.cpp) over the fake
// runtime's ordered mode (hip_fake.cpp: every stream a queue that runs at forcing points only, in an order the schedule chooses),
// under AddressSanitizer / UBSan, no GPU: `make order_test`, tests/test_host_order.py.
//
// Every case runs with everything completing at once and under the three lazy schedules, and must give the same bytes each time.
// What the bytes are compared with: for the readers that move data (sixdof_watch_read, sixdof_history_stream, sixdof_history_read)
// and for the extremes of case a, a plain loop over the fixture's host copy of every upload; for the reductions, a blocking read
// of the same ticks with everything completing at once, on a twin handle that was fed the same uploads and whose ring is long
// enough to hold them all — the blocking at-once reads themselves are pinned to plain loops by the five reader programs.
// The cases:
//   a  the call sequence of the GPU test that once faulted, in a process with other handles before, during and after it
//   b  two asynchronous reads in flight with an overwriting step between them, per reader
//   c  the second read grows the staging buffer (and the scratch) under the pending first
//   d  the same host pointer, a longer second read, then sixdof_sync: no lock left, none too short for its copy
//   e  a blocking read into a buffer that a pending asynchronous read page-locked
//   f  HOLD, HOLD | CONTINUE, CONTINUE | ASYNC with overwriting steps between, against one call, under forced segment counts
//   g  sixdof_set_history, sixdof_bind_columns, sixdof_set_watch and sixdof_destroy under a pending asynchronous read
//   h  the buffer lifetimes of HipExec.stream_envelope, stream_covariance and _stream_accumulate (elodin_amd/exec.py)
// One line per case and schedule: `order: <case> <schedule>: ok`.
#include "ring_host_fixture.hpp"
#include "covariance_plan.hpp"
#include "extremes_plan.hpp"

namespace {

using sixdof::QuantileBits;
using Bufs = std::vector<std::vector<double>>;
constexpr uint64_t kRows = 60, kRing = 8, kLong = 32;
constexpr uint32_t kPeriod = 4;

// A handle of n f64 rows without edges — the per-entity path, whose (fake) step launch records — and a ring from tick 1 on.
// step(ticks) rewrites and uploads the columns first, so every tick of that batch holds that upload; step(ticks, false) steps on
// what the device holds, without the upload's synchronisation.  Every upload is kept: at(k, tick) is what tick holds of column k.
struct Sim {
    uint64_t n, tick = 0;
    sixdof_handle* h = nullptr;
    std::vector<uint64_t> ids;
    std::vector<double> col[5];
    std::vector<sixdof_column> cols;
    std::vector<std::vector<double>> upload[4];
    std::vector<size_t> upload_of_tick;
    std::mt19937_64 rng;

    Sim(uint64_t n_, uint64_t ring, uint64_t seed, uint32_t ticks_per_launch = 1) : n(n_), rng(seed) {
        for (uint64_t i = 0; i < n; i++) ids.push_back(i + 1);
        sixdof_desc d{};
        d.struct_size = sizeof(d), d.integrator = SIXDOF_INTEGRATOR_RK4, d.simulation_time_step = 1.0 / 120.0, d.ticks_per_launch = ticks_per_launch;
        d.dtype = SIXDOF_F64, d.n_entities = n;
        for (int k = 0; k < 5; k++) {
            const uint64_t w = k < 4 ? kWidths[k] : 7;
            col[k].assign(n * w, 1.0);
            sixdof_column c{};
            c.component_id = sixdof_component_id(k < 4 ? kNames[k] : "inertia"), c.prim_type = SIXDOF_PRIM_F64;
            c.ndim = 1, c.dims[0] = w, c.n_rows = n, c.entity_ids = ids.data(), c.host_ptr = col[k].data();
            cols.push_back(c);
        }
        const bool ok = sixdof_create(&d, &h) == SIXDOF_OK && sixdof_bind_columns(h, cols.data(), cols.size()) == SIXDOF_OK && sixdof_upload(h) == SIXDOF_OK &&
                        (!ring || sixdof_set_history(h, static_cast<uint32_t>(ring)) == SIXDOF_OK);
        if (!ok) complain(std::string("setup: ") + (h ? sixdof_last_error(h) : sixdof_last_error(nullptr)));
    }
    bool step(uint64_t ticks, bool fresh = true) {
        if (fresh || upload[0].empty()) {
            std::normal_distribution<double> normal(0.0, 1.0);
            for (int k = 0; k < 4; k++) {
                for (double& x : col[k]) x = normal(rng) + 0.01 * static_cast<double>(upload[0].size());
                upload[k].push_back(col[k]);
            }
            if (sixdof_upload(h) != SIXDOF_OK) return complain(std::string("upload: ") + sixdof_last_error(h)), false;
        }
        if (sixdof_step(h, ticks, nullptr) != SIXDOF_OK) return complain(std::string("step: ") + sixdof_last_error(h)), false;
        for (uint64_t t = 0; t < ticks; t++) upload_of_tick.push_back(upload[0].size() - 1);
        tick += ticks;
        return true;
    }
    bool steps(uint64_t batches, uint64_t ticks) {
        for (uint64_t b = 0; b < batches; b++)
            if (!step(ticks)) return false;
        return true;
    }
    const std::vector<double>& at(int k, uint64_t t) const { return upload[k][upload_of_tick[t - 1]]; }
    void destroy() { sixdof_destroy(h), h = nullptr; }
    ~Sim() { destroy(); }
};

struct Flags { bool async = false, hold = false, cont = false; };

// One of the seven readers.  sizes(n, samples, big): doubles of every buffer it fills; read(s, first, samples, out, flags, big):
// the samples first, first + 1, ... into out (at least that large), `big`: the scans' larger request (more and wider components,
// more triggers and a capture) — the other readers grow with the samples.  truth: the expected buffers as a plain loop, if one is easy.
struct Reader {
    const char* name;
    std::function<int(const Sim&)> setup;
    std::function<std::vector<size_t>(uint64_t n, uint64_t samples, bool big)> sizes;
    std::function<int(const Sim&, uint64_t first, uint64_t samples, Bufs& out, Flags f, bool big)> read;
    std::function<Bufs(const Sim&, uint64_t first, uint64_t samples)> truth;
    const char* segments_env = nullptr;   // a scan
};

const uint64_t kWatched[3] = {3, 5, kRows};

std::vector<double*> pointers(Bufs& out) {
    std::vector<double*> p;
    for (auto& b : out) p.push_back(b.data());
    return p;
}

const Reader kWatch{
    "watch",
    [](const Sim& s) {
        const uint64_t comp[2] = {sixdof_component_id("world_pos"), sixdof_component_id("world_vel")};
        return sixdof_set_watch(s.h, comp, 2, kWatched, 3);
    },
    [](uint64_t, uint64_t samples, bool) { return std::vector<size_t>{3 * samples * 7, 3 * samples * 6}; },
    [](const Sim& s, uint64_t first, uint64_t samples, Bufs& out, Flags f, bool) {
        void* dst[2] = {out[0].data(), out[1].data()};
        return sixdof_watch_read(s.h, first, samples, 1, dst, f.async ? SIXDOF_WATCH_ASYNC : 0u);
    },
    [](const Sim& s, uint64_t first, uint64_t samples) {
        Bufs want(2);
        for (int k = 0; k < 2; k++)
            for (uint64_t e = 0; e < 3; e++)
                for (uint64_t j = 0; j < samples; j++)
                    for (uint64_t c = 0; c < kWidths[k]; c++) want[k].push_back(s.at(k, first + j)[(kWatched[e] - 1) * kWidths[k] + c]);
        return want;
    }};

const Reader kStream{
    "stream", {},
    [](uint64_t n, uint64_t samples, bool) { return std::vector<size_t>{samples * n * 7, samples * n * 6, samples * n * 6, samples * n * 6}; },
    [](const Sim& s, uint64_t first, uint64_t samples, Bufs& out, Flags f, bool) {
        void* dst[4] = {out[0].data(), out[1].data(), out[2].data(), out[3].data()};
        if (f.async) return sixdof_history_stream(s.h, first, samples, dst);
        for (int k = 0; k < 4; k++)      // the blocking counterpart: one sixdof_history_read per tick and column
            for (uint64_t j = 0; j < samples; j++)
                if (int rc = sixdof_history_read(s.h, sixdof_component_id(kNames[k]), first + j, out[k].data() + j * s.n * kWidths[k]); rc != SIXDOF_OK) return rc;
        return int(SIXDOF_OK);
    },
    [](const Sim& s, uint64_t first, uint64_t samples) {
        Bufs want(4);
        for (int k = 0; k < 4; k++)
            for (uint64_t j = 0; j < samples; j++) want[k].insert(want[k].end(), s.at(k, first + j).begin(), s.at(k, first + j).end());
        return want;
    }};

const Reader kEnvelope{
    "envelope", {},
    [](uint64_t, uint64_t samples, bool) { return std::vector<size_t>{samples * kPeriod * 5 * 7, samples * kPeriod * 5 * 6}; },
    [](const Sim& s, uint64_t first, uint64_t samples, Bufs& out, Flags f, bool) {
        const uint64_t comp[2] = {sixdof_component_id("world_pos"), sixdof_component_id("force")};
        return sixdof_history_envelope(s.h, comp, 2, first, samples, 1, kPeriod, pointers(out).data(), f.async ? SIXDOF_ENVELOPE_ASYNC : 0u);
    },
    {}};

const Reader kQuantiles{
    "quantiles", {},
    [](uint64_t, uint64_t samples, bool) { return std::vector<size_t>{samples * kPeriod * 7 * 7, samples * kPeriod * 7 * 6}; },
    [](const Sim& s, uint64_t first, uint64_t samples, Bufs& out, Flags f, bool) {
        const uint64_t comp[2] = {sixdof_component_id("world_pos"), sixdof_component_id("force")};
        const uint32_t num[3] = {0, 1, 2};
        return sixdof_history_quantiles(s.h, comp, 2, first, samples, 1, kPeriod, num, 2, 3, pointers(out).data(), f.async ? SIXDOF_QUANTILE_ASYNC : 0u);
    },
    {}};

const Reader kCovariance{
    "covariance", {},
    [](uint64_t, uint64_t samples, bool) { return std::vector<size_t>{samples * kPeriod * sixdof::covariance_fields(3)}; },
    [](const Sim& s, uint64_t first, uint64_t samples, Bufs& out, Flags f, bool) {
        const sixdof_cov_channel ch[3] = {{sixdof_component_id("world_vel"), 0, 0}, {sixdof_component_id("world_vel"), 2, 0}, {sixdof_component_id("world_pos"), 1, 0}};
        return sixdof_history_covariance(s.h, ch, 3, first, samples, 1, kPeriod, out[0].data(), f.async ? SIXDOF_COVARIANCE_ASYNC : 0u);
    },
    {}};

// the six planes [6][n * w] of column k over the ticks first, first + every, ...: a plain loop over what was uploaded
std::vector<double> extremes_loop(const Sim& s, int k, uint64_t first, uint64_t samples, uint64_t every) {
    using B = QuantileBits<double>;
    const uint64_t total = s.n * kWidths[k];
    std::vector<double> out(SIXDOF_EXTREMES_PLANES * total);
    for (uint64_t i = 0; i < total; i++) {
        uint64_t count = 0, key_min = 0, key_max = 0, tick_min = 0, tick_max = 0, first_nonfinite = 0;
        double min = std::numeric_limits<double>::quiet_NaN(), max = min;
        for (uint64_t j = 0; j < samples; j++) {
            const uint64_t tick = first + j * every;
            const double x = s.at(k, tick)[i];
            if (!std::isfinite(x)) {
                if (!first_nonfinite) first_nonfinite = tick;
                continue;
            }
            const uint64_t key = B::key(B::raw(x));
            if (count == 0 || key < key_min) key_min = key, min = x, tick_min = tick;
            if (count == 0 || key > key_max) key_max = key, max = x, tick_max = tick;
            count++;
        }
        const double planes[SIXDOF_EXTREMES_PLANES] = {double(count), min, double(tick_min), max, double(tick_max), double(first_nonfinite)};
        for (size_t p = 0; p < SIXDOF_EXTREMES_PLANES; p++) out[p * total + i] = planes[p];
    }
    return out;
}

const Reader kExtremes{
    "extremes", {},
    [](uint64_t n, uint64_t, bool big) { return big ? std::vector<size_t>{6 * n * 7, 6 * n * 6} : std::vector<size_t>{6 * n * 6}; },
    [](const Sim& s, uint64_t first, uint64_t samples, Bufs& out, Flags f, bool big) {
        const uint64_t small_comp[1] = {sixdof_component_id("world_vel")}, big_comp[2] = {sixdof_component_id("world_pos"), sixdof_component_id("force")};
        const uint32_t flags = (f.async ? SIXDOF_EXTREMES_ASYNC : 0u) | (f.hold ? SIXDOF_EXTREMES_HOLD : 0u) | (f.cont ? SIXDOF_EXTREMES_CONTINUE : 0u);
        return sixdof_history_extremes(s.h, big ? big_comp : small_comp, big ? 2 : 1, first, samples, 1, f.hold ? nullptr : pointers(out).data(), flags);
    },
    {}, "SIXDOF_EXTREMES_SEGMENTS"};

const Reader kEvents{
    "events", {},
    [](uint64_t n, uint64_t, bool big) {
        return big ? std::vector<size_t>{n / kPeriod * 2 * SIXDOF_EVENTS_PLANES, n * 2 * 7} : std::vector<size_t>{n / kPeriod * 1 * SIXDOF_EVENTS_PLANES};
    },
    [](const Sim& s, uint64_t first, uint64_t samples, Bufs& out, Flags f, bool big) {
        const sixdof_event_trigger trig[2] = {{sixdof_component_id("world_vel"), 2, 1, SIXDOF_EVENT_GT, SIXDOF_EVENT_LEVEL, 0.75},
                                              {sixdof_component_id("force"), 5, 3, SIXDOF_EVENT_LT, SIXDOF_EVENT_CROSSING, -0.25}};
        const uint64_t capture[1] = {sixdof_component_id("world_pos")};
        const uint32_t flags = (f.async ? SIXDOF_EVENTS_ASYNC : 0u) | (f.hold ? SIXDOF_EVENTS_HOLD : 0u) | (f.cont ? SIXDOF_EVENTS_CONTINUE : 0u);
        double* cap[1] = {big && !f.hold ? out[1].data() : nullptr};
        return sixdof_history_events(s.h, trig, big ? 2 : 1, capture, big ? 1 : 0, kPeriod, first, samples, 1, f.hold ? nullptr : out[0].data(), cap, flags);
    },
    {}, "SIXDOF_EVENTS_SEGMENTS"};

const Reader* const kReaders[7] = {&kWatch, &kStream, &kEnvelope, &kQuantiles, &kCovariance, &kExtremes, &kEvents};

Bufs make(const std::vector<size_t>& sizes, double fill = -7.0) {
    Bufs b;
    for (size_t s : sizes) b.emplace_back(s, fill);
    return b;
}
// got holds want in the leading doubles of every buffer (the buffers of a case may be larger than the read that is checked)
void expect_same(const std::string& what, const Bufs& got, const Bufs& want) {
    if (got.size() < want.size()) return complain(what + ": fewer buffers than expected");
    for (size_t k = 0; k < want.size(); k++) {
        if (got[k].size() < want[k].size()) return complain(what + ": buffer " + std::to_string(k) + " is too short");
        for (size_t i = 0; i < want[k].size(); i++)
            if (std::memcmp(&got[k][i], &want[k][i], 8) != 0)
                return complain(what + ": buffer " + std::to_string(k) + " double " + std::to_string(i) + " of " + std::to_string(want[k].size()) + ": " +
                                std::to_string(got[k][i]) + " != " + std::to_string(want[k][i]));
    }
}
void expect_unlocked(const std::string& what, const Bufs& bufs) {
    for (size_t k = 0; k < bufs.size(); k++)
        if (hip_fake::lock_intersects(bufs[k].data(), bufs[k].size() * sizeof(double))) complain(what + ": a page lock still intersects buffer " + std::to_string(k));
}
void ok(const std::string& what, int rc, const Sim& s) {
    if (rc != SIXDOF_OK) complain(what + ": status " + std::to_string(rc) + ": " + sixdof_last_error(s.h));
}

// What the reads of a case have to return: blocking reads with everything completing at once, on a twin whose ring holds every
// tick; where the reader has a plain loop, the twin's read is checked against it too.
struct Want {
    uint64_t first, samples;
    bool big;
    Bufs bufs;
};
void reference(const Reader& r, uint64_t seed, const std::function<void(Sim&)>& run, std::vector<Want>& wants) {
    hip_fake::set_schedule(hip_fake::kAtOnce);
    Sim twin(kRows, kLong, seed);
    if (r.setup) ok(std::string(r.name) + ": twin setup", r.setup(twin), twin);
    run(twin);
    for (Want& w : wants) {
        w.bufs = make(r.sizes(kRows, w.samples, w.big));
        ok(std::string(r.name) + ": twin read", r.read(twin, w.first, w.samples, w.bufs, Flags{}, w.big), twin);
        if (r.truth) expect_same(std::string(r.name) + ": the twin's read against the plain loop", w.bufs, r.truth(twin, w.first, w.samples));
    }
}

// ---- a. the recorded sequence --------------------------------------------------------------------------------------------
// 4,099 rows in f64 without edges, 7 ticks per launch, a ring of 64, 50 ticks; the extremes of the four columns at ticks 1, 8, ..
// 50, every tick of every column read back, the extremes of world_vel at tick 50 alone; with a 300-row handle created, used and
// destroyed while the first lives, and another after it.
void small_neighbour(const std::string& what) {
    Sim s(300, 16, 300);
    if (!s.steps(4, 4)) return;
    Bufs out = make(kExtremes.sizes(300, 8, true));
    ok(what, kExtremes.read(s, 9, 8, out, Flags{true}, true), s);
    ok(what, sixdof_download_wait(s.h), s);
    Bufs want{extremes_loop(s, 0, 9, 8, 1), extremes_loop(s, 3, 9, 8, 1)};
    expect_same(what, out, want);
    ok(what, sixdof_sync(s.h), s);
    expect_unlocked(what, out);
}
void case_a(int schedule) {
    hip_fake::set_schedule(schedule);
    {
        Sim s(4099, 64, 4099, 7);
        if (!s.steps(5, 10)) return;
        small_neighbour("a: the second handle");
        const uint64_t comp[4] = {sixdof_component_id(kNames[0]), sixdof_component_id(kNames[1]), sixdof_component_id(kNames[2]), sixdof_component_id(kNames[3])};
        Bufs out = make({6 * s.n * 7, 6 * s.n * 6, 6 * s.n * 6, 6 * s.n * 6}), want;
        ok("a: extremes", sixdof_history_extremes(s.h, comp, 4, 1, 8, 7, pointers(out).data(), 0), s);
        for (int k = 0; k < 4; k++) want.push_back(extremes_loop(s, k, 1, 8, 7));
        expect_same("a: extremes of ticks 1, 8, .. 50", out, want);
        std::vector<double> block(s.n * 7);
        for (int k = 0; k < 4; k++)
            for (uint64_t t = 1; t <= 50; t++) {
                ok("a: history_read", sixdof_history_read(s.h, comp[k], t, block.data()), s);
                if (std::memcmp(block.data(), s.at(k, t).data(), s.n * kWidths[k] * 8) != 0) return complain(std::string("a: history_read of ") + kNames[k] + " at tick " + std::to_string(t));
            }
        Bufs one = make({6 * s.n * 6});
        ok("a: extremes of one tick", sixdof_history_extremes(s.h, comp + 1, 1, 50, 1, 1, pointers(one).data(), 0), s);
        expect_same("a: extremes of world_vel at tick 50", one, Bufs{extremes_loop(s, 1, 50, 1, 1)});
    }
    small_neighbour("a: the third handle");
}

// ---- b. two reads in flight ----------------------------------------------------------------------------------------------
// Ticks 1 .. 8 fill the ring.  Read A takes ticks 3 .. 6 asynchronously and read A' ticks 7 .. 8, so that the newest pending read
// is not the one in the way; with no wait a step of four ticks overwrites the slots of ticks 1 .. 4 — accepted: the ring is read
// on the compute stream, and where the copy stream reads it (sixdof_history_stream) the step is held back on the device; read B
// takes ticks 9 .. 12 into other buffers; one wait; all three are their own ticks.
void case_b(const Reader& r, int schedule) {
    std::vector<Want> want{{3, 4, false, {}}, {9, 4, false, {}}, {7, 2, false, {}}};
    reference(r, 11, [](Sim& t) { t.steps(4, 2) && t.step(4, false); }, want);
    hip_fake::set_schedule(schedule);
    Sim s(kRows, kRing, 11);
    if (r.setup) ok("setup", r.setup(s), s);
    if (!s.steps(4, 2)) return;
    Bufs a = make(r.sizes(kRows, 4, false)), b = make(r.sizes(kRows, 4, false), -9.0);
    Bufs a2 = make(r.sizes(kRows, 2, false), -8.0);
    ok("read A", r.read(s, 3, 4, a, Flags{true}, false), s);
    ok("read A'", r.read(s, 7, 2, a2, Flags{true}, false), s);
    if (!s.step(4, false)) return;
    ok("read B", r.read(s, 9, 4, b, Flags{true}, false), s);
    ok("download_wait", sixdof_download_wait(s.h), s);
    expect_same("read A after the overwriting step", a, want[0].bufs);
    expect_same("read A'", a2, want[2].bufs);
    expect_same("read B", b, want[1].bufs);
    ok("sync", sixdof_sync(s.h), s);
    expect_unlocked("after sync: A", a), expect_unlocked("after sync: A'", a2), expect_unlocked("after sync: B", b);
}

// ---- c. growth under a pending copy ----------------------------------------------------------------------------------------
// Read A: ticks 5 .. 6, the small request.  Read B, at once: ticks 3 .. 8, the large one — more samples, more and wider components —
// which needs a larger staging buffer and, where the reader has one, more scratch.
void case_c(const Reader& r, int schedule) {
    std::vector<Want> want{{5, 2, false, {}}, {3, 6, true, {}}};
    reference(r, 12, [](Sim& t) { t.steps(4, 2); }, want);
    hip_fake::set_schedule(schedule);
    Sim s(kRows, kRing, 12);
    if (r.setup) ok("setup", r.setup(s), s);
    if (!s.steps(4, 2)) return;
    Bufs a = make(r.sizes(kRows, 2, false)), b = make(r.sizes(kRows, 6, true), -9.0);
    if (r.segments_env) force_segments(r.segments_env, 1);   // the scans: no scratch for A, scratch for the three segments of B
    ok("read A", r.read(s, 5, 2, a, Flags{true}, false), s);
    if (r.segments_env) force_segments(r.segments_env, 3);
    ok("read B", r.read(s, 3, 6, b, Flags{true}, true), s);
    if (r.segments_env) force_segments(r.segments_env, 0);
    ok("download_wait", sixdof_download_wait(s.h), s);
    expect_same("read A after B grew the buffers", a, want[0].bufs);
    expect_same("read B", b, want[1].bufs);
    ok("sync", sixdof_sync(s.h), s);
}

// ---- d. same pointer, longer read ------------------------------------------------------------------------------------------
// Read A into p, with no synchronisation the longer read B into the same p, then sixdof_sync: B's values, complete; no copy under
// a lock shorter than itself (the fake says so); no lock left over the buffers.
void case_d(const Reader& r, int schedule) {
    std::vector<Want> want{{3, 6, true, {}}};
    reference(r, 13, [](Sim& t) { t.steps(4, 2); }, want);
    hip_fake::set_schedule(schedule);
    Sim s(kRows, kRing, 13);
    if (r.setup) ok("setup", r.setup(s), s);
    if (!s.steps(4, 2)) return;
    Bufs p = make(r.sizes(kRows, 6, true));
    ok("read A", r.read(s, 5, 2, p, Flags{true}, false), s);
    ok("read B", r.read(s, 3, 6, p, Flags{true}, true), s);
    ok("sync", sixdof_sync(s.h), s);
    expect_same("the longer read into the same pointer", p, want[0].bufs);
    expect_unlocked("after sync", p);
}

// ---- e. blocking after asynchronous ----------------------------------------------------------------------------------------
// Read A asynchronously into p, then the longer read B, blocking, into the same p: B's values when B returns, and still after the
// wait and the sync.  (sixdof_history_stream has no blocking form and nothing that orders a sixdof_history_read behind its copies:
// there the caller waits for A first, which leaves the lock in place.)
void case_e(const Reader& r, int schedule) {
    std::vector<Want> want{{3, 6, true, {}}};
    reference(r, 14, [](Sim& t) { t.steps(4, 2); }, want);
    hip_fake::set_schedule(schedule);
    Sim s(kRows, kRing, 14);
    if (r.setup) ok("setup", r.setup(s), s);
    if (!s.steps(4, 2)) return;
    Bufs p = make(r.sizes(kRows, 6, true));
    ok("read A", r.read(s, 5, 2, p, Flags{true}, false), s);
    if (&r == &kStream) ok("download_wait before B", sixdof_download_wait(s.h), s);
    ok("read B", r.read(s, 3, 6, p, Flags{}, true), s);
    expect_same("the blocking read when it returns", p, want[0].bufs);
    ok("download_wait", sixdof_download_wait(s.h), s);
    ok("sync", sixdof_sync(s.h), s);
    expect_same("the blocking read after the wait", p, want[0].bufs);
    expect_unlocked("after sync", p);
}

// ---- f. the scans' flags ---------------------------------------------------------------------------------------------------
// Ticks 1 .. 8 held, 9 .. 16 held and continued, 17 .. 24 continued and delivered asynchronously, with the eight ticks between the
// calls overwriting every slot already accumulated: one blocking call over ticks 1 .. 24 of a ring that holds them all.
void case_f(const Reader& r, uint64_t segments, int schedule) {
    std::vector<Want> want{{1, 24, true, {}}};
    reference(r, 15, [](Sim& t) { t.steps(12, 2); }, want);
    hip_fake::set_schedule(schedule);
    force_segments(r.segments_env, segments);
    Sim s(kRows, kRing, 15);
    Bufs out = make(r.sizes(kRows, 8, true));
    bool fine = s.steps(4, 2);
    if (fine) ok("HOLD", r.read(s, 1, 8, out, Flags{false, true, false}, true), s);
    fine = fine && s.steps(4, 2);
    if (fine) ok("HOLD | CONTINUE", r.read(s, 9, 8, out, Flags{false, true, true}, true), s);
    fine = fine && s.steps(4, 2);
    if (fine) ok("CONTINUE | ASYNC", r.read(s, 17, 8, out, Flags{true, false, true}, true), s);
    force_segments(r.segments_env, 0);
    ok("download_wait", sixdof_download_wait(s.h), s);
    expect_same("three calls against one", out, want[0].bufs);
    ok("sync", sixdof_sync(s.h), s);
}

// ---- g. teardown under load --------------------------------------------------------------------------------------------------
// An asynchronous read of ticks 3 .. 6 is pending when the ring is re-sized or dropped, the columns are bound again, the watch is
// replaced or the handle is destroyed.  No violation; the buffers are complete after the documented wait (sixdof_destroy: when it
// returns), unless the call was refused.
const char* const kTeardowns[5] = {"set_history", "set_history_0", "bind_columns", "set_watch", "destroy"};
void case_g(const Reader& r, int op, int schedule) {
    std::vector<Want> want{{3, 4, false, {}}};
    reference(r, 16, [](Sim& t) { t.steps(4, 2); }, want);
    hip_fake::set_schedule(schedule);
    Sim s(kRows, kRing, 16);
    if (r.setup) ok("setup", r.setup(s), s);
    if (!s.steps(4, 2)) return;
    Bufs a = make(r.sizes(kRows, 4, false));
    ok("read A", r.read(s, 3, 4, a, Flags{true}, false), s);
    const uint64_t pos = sixdof_component_id("world_pos"), two[2] = {1, 2};
    int rc = SIXDOF_OK;
    switch (op) {
    case 0: rc = sixdof_set_history(s.h, 12); break;
    case 1: rc = sixdof_set_history(s.h, 0); break;
    case 2: rc = sixdof_bind_columns(s.h, s.cols.data(), s.cols.size()); break;
    case 3: rc = sixdof_set_watch(s.h, &pos, 1, two, 2); break;
    default: s.destroy(); break;
    }
    if (rc != SIXDOF_OK && !*sixdof_last_error(s.h)) complain(std::string(kTeardowns[op]) + " was refused without a message");
    if (s.h) ok("download_wait", sixdof_download_wait(s.h), s);
    expect_same(std::string("read A after ") + kTeardowns[op], a, want[0].bufs);
    s.destroy();
    expect_unlocked("after sixdof_destroy", a);
}

// ---- h. buffer lifetime as Python uses it ------------------------------------------------------------------------------------
// HipExec.stream_envelope and stream_covariance (elodin_amd/exec.py): _stream_reduce (lines 633-648) and stream_covariance
// (812-829) make two buffer sets, call sync() (645, 826) and enter _stream_batches (1024-1049), mirrored line by line below.  The
// arrays are locals of those functions: they are let go when _stream_batches has returned, after the sync() of its finally clause.
void case_h_batches(const Reader& r, int schedule) {
    constexpr uint64_t kBatches = 5, kTicks = 4;
    std::vector<Want> want;
    for (uint64_t i = 0; i < kBatches; i++) want.push_back({1 + i * kTicks, kTicks, false, {}});
    reference(r, 17, [](Sim& t) { t.steps(kBatches, kTicks); }, want);
    hip_fake::set_schedule(schedule);
    Sim s(kRows, kTicks, 17);                                       // 641-642 / 823-824: a ring one batch deep
    Bufs raw[2] = {make(r.sizes(kRows, kTicks, false)), make(r.sizes(kRows, kTicks, false))};   // 643 / 825
    ok("sync", sixdof_sync(s.h), s);                                // 645 / 826
    ok("set_flags", sixdof_set_flags(s.h, SIXDOF_FLAG_ASYNC_STEP), s);   // 1031
    uint64_t first[kBatches];
    for (uint64_t i = 0; i < kBatches; i++) {                       // 1035
        first[i] = s.tick + 1;                                      // 1036
        if (!s.step(kTicks)) return;                                // 1037: invoke_batch (the upload is the fixture's: the fake computes nothing)
        if (i > 0) {
            ok("download_wait", sixdof_download_wait(s.h), s);      // 1039
            expect_same("batch " + std::to_string(i - 1) + " when it is consumed", raw[(i - 1) % 2], want[i - 1].bufs);   // 1041
        }
        ok("read", r.read(s, first[i], kTicks, raw[i % 2], Flags{true}, false), s);   // 1042
    }
    ok("download_wait", sixdof_download_wait(s.h), s);              // 1043
    expect_same("the last batch", raw[(kBatches - 1) % 2], want[kBatches - 1].bufs);   // 1045
    ok("set_flags", sixdof_set_flags(s.h, 0), s);                   // 1047
    ok("sync", sixdof_sync(s.h), s);                                // 1048
    expect_unlocked("when the arrays go", raw[0]), expect_unlocked("when the arrays go", raw[1]);
}
// HipExec.stream_extremes (868-884) through _stream_accumulate (886-906): one buffer set, held calls, the last one blocking.
void case_h_accumulate(int schedule) {
    constexpr uint64_t kBatches = 5, kTicks = 4;
    const Reader& r = kExtremes;
    std::vector<Want> want{{1, kBatches * kTicks, true, {}}};
    reference(r, 18, [](Sim& t) { t.steps(kBatches, kTicks); }, want);
    hip_fake::set_schedule(schedule);
    Sim s(kRows, kTicks, 18);                                       // 892-893
    Bufs raw = make(r.sizes(kRows, kTicks, true));                  // 880
    ok("sync", sixdof_sync(s.h), s);                                // 894
    ok("set_flags", sixdof_set_flags(s.h, SIXDOF_FLAG_ASYNC_STEP), s);   // 895
    for (uint64_t i = 0; i < kBatches; i++) {                       // 898
        const uint64_t first = s.tick + 1;                          // 899
        if (!s.step(kTicks)) break;                                 // 900
        const bool last = i + 1 == kBatches;                        // 901
        ok("read", r.read(s, first, kTicks, raw, Flags{false, !last, i != 0}, true), s);   // 902
    }
    ok("set_flags", sixdof_set_flags(s.h, 0), s);                   // 904
    ok("sync", sixdof_sync(s.h), s);                                // 905
    expect_same("five batches against one call", raw, want[0].bufs);
    expect_unlocked("when the arrays go", raw);
}

// One case under one schedule: nothing new complained of, no violation, nothing left alive or queued.
void run(const std::string& name, int schedule, const std::function<void(int)>& body) {
    const int failures0 = g_failures;
    const long violations0 = hip_fake::violations();
    body(schedule);
    if (hip_fake::queued()) complain("operations are still queued after the last handle was destroyed");
    hip_fake::set_schedule(hip_fake::kAtOnce);
    if (hip_fake::violations() != violations0) complain(std::to_string(hip_fake::violations() - violations0) + " violations reported by the fake runtime");
    if (hip_fake::live_allocations() || hip_fake::live_streams() || hip_fake::live_events() || hip_fake::live_page_locks()) complain("something outlives sixdof_destroy");
    const bool fine = g_failures == failures0;
    if (!fine) std::fprintf(stderr, "  ^ in case %s under the %s schedule\n", name.c_str(), hip_fake::schedule_name(schedule));
    std::printf("order: %s %s: %s\n", name.c_str(), hip_fake::schedule_name(schedule), fine ? "ok" : "FAILED");
}

}  // namespace

int main() {
    for (int schedule : {int(hip_fake::kAtOnce), int(hip_fake::kMinimal), int(hip_fake::kComputeFirst), int(hip_fake::kCopyFirst)}) {
        run("a", schedule, case_a);
        for (const Reader* r : kReaders) run(std::string("b-") + r->name, schedule, [&](int s) { case_b(*r, s); });
        for (const Reader* r : kReaders) run(std::string("c-") + r->name, schedule, [&](int s) { case_c(*r, s); });
        for (const Reader* r : kReaders) run(std::string("d-") + r->name, schedule, [&](int s) { case_d(*r, s); });
        for (const Reader* r : kReaders) run(std::string("e-") + r->name, schedule, [&](int s) { case_e(*r, s); });
        for (const Reader* r : {&kExtremes, &kEvents})
            for (uint64_t segments : {uint64_t(1), uint64_t(2), uint64_t(sixdof::kScanLoads + 2)})
                run(std::string("f-") + r->name + "-" + std::to_string(segments), schedule, [&](int s) { case_f(*r, segments, s); });
        for (int op = 0; op < 5; op++)
            for (const Reader* r : {&kWatch, &kStream, &kEnvelope}) run(std::string("g-") + kTeardowns[op] + "-" + r->name, schedule, [&](int s) { case_g(*r, op, s); });
        run("h-envelope", schedule, [&](int s) { case_h_batches(kEnvelope, s); });
        run("h-covariance", schedule, [&](int s) { case_h_batches(kCovariance, s); });
        run("h-extremes", schedule, case_h_accumulate);
    }
    return verdict("order_host_test");
}
