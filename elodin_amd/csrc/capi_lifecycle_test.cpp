// capi_lifecycle_test.cpp — the C ABI's host layer (sixdof_capi.cpp) against a fake runtime (hip_fake.cpp) under
// AddressSanitizer / UBSan, no GPU: `make capi_test`, tests/test_capi_lifecycle_host.py.
//
// One scenario walks the life of a handle at eight entities.  It runs once without a fault, which counts the runtime
// calls that can fail (N) and records what every read returned; then N times with call k failing.  Each time exactly one
// step must return a status with a message, succeed when called again, and the rest of the scenario must return what
// the fault-free run returned; after sixdof_destroy nothing of the runtime's may be left alive.  Three named cases pin
// the defects that motivated the owners of device_mem.hpp.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../include/sixdof_hip.h"

namespace hip_fake {
void fail_after(long n);   // the n-th fallible call from now fails, once (0: the next one; < 0: none)
bool fired();
long calls();
long violations();
size_t live_allocations();
size_t live_streams();
size_t live_events();
size_t live_page_locks();
enum { kAtOnce = 0, kMinimal = 1, kComputeFirst = 2, kCopyFirst = 3 };   // the ordered mode: hip_fake.cpp
void set_schedule(int schedule);
const char* schedule_name(int schedule);
}  // namespace hip_fake

namespace {

constexpr uint64_t kN = 8;
int g_failures = 0;
const char* g_program = "build/capi_fake_program.so";

void complain(const std::string& what) {
    std::fprintf(stderr, "FAIL: %s\n", what.c_str());
    g_failures++;
}

// The host side of one run: the caller's column buffers and every buffer a read fills.
struct World {
    std::vector<uint64_t> body_ids, extra_ids;
    std::vector<double> pos, vel, accel, force, inertia, extra, extra_wide;
    std::vector<double> hist_pos, hist_extra, stream[4], watch_pos[2], watch_extra[2];
    std::vector<uint32_t> edge_rows;
    std::vector<uint8_t> flags;
    uint64_t nonfinite = ~0ull, tick = 0;

    World() {
        for (uint64_t i = 0; i < kN; i++) body_ids.push_back(i + 1);
        for (uint64_t i = 0; i < kN + 2; i++) extra_ids.push_back(kN + 2 - i);   // another entity set, another order: a joined column
        auto fill = [](std::vector<double>& v, size_t n, double base) {
            v.resize(n);
            for (size_t i = 0; i < n; i++) v[i] = base + 0.25 * static_cast<double>(i);
        };
        fill(pos, kN * 7, 1.0), fill(vel, kN * 6, 2.0), fill(accel, kN * 6, 3.0), fill(force, kN * 6, 4.0), fill(inertia, kN * 7, 5.0);
        fill(extra, (kN + 2) * 2, 6.0), fill(extra_wide, (kN + 2) * 6, 7.0);
    }
    std::vector<sixdof_column> columns(bool wide) {
        auto col = [&](const char* name, uint64_t w, std::vector<double>& v, std::vector<uint64_t>& ids) {
            sixdof_column c{};
            c.component_id = sixdof_component_id(name), c.prim_type = SIXDOF_PRIM_F64, c.ndim = 1, c.dims[0] = w;
            c.n_rows = ids.size(), c.entity_ids = ids.data(), c.host_ptr = v.data();
            return c;
        };
        return {col("world_pos", 7, pos, body_ids),   col("world_vel", 6, vel, body_ids), col("world_accel", 6, accel, body_ids),
                col("force", 6, force, body_ids),     col("inertia", 7, inertia, body_ids),
                wide ? col("extra", 6, extra_wide, extra_ids) : col("extra", 2, extra, extra_ids)};
    }
    uint64_t digest() const {
        uint64_t hsh = 1469598103934665603ull;
        auto mix = [&](const void* p, size_t bytes) {
            for (size_t i = 0; i < bytes; i++) hsh = (hsh ^ static_cast<const unsigned char*>(p)[i]) * 1099511628211ull;
        };
        for (auto* v : {&pos, &vel, &accel, &force, &inertia, &extra, &extra_wide, &hist_pos, &hist_extra, &stream[0], &stream[1], &stream[2],
                        &stream[3], &watch_pos[0], &watch_pos[1], &watch_extra[0], &watch_extra[1]})
            mix(v->data(), v->size() * sizeof(double));
        mix(edge_rows.data(), edge_rows.size() * sizeof(uint32_t));
        mix(flags.data(), flags.size());
        mix(&nonfinite, 8), mix(&tick, 8);
        return hsh;
    }
};

// One run of the scenario.  A step that fails must have been hit by the injected fault and say why; it is called again
// (`again`, by default the step itself) without a fault and must then succeed.
struct Run {
    World w;
    sixdof_handle* h = nullptr;
    int failed_steps = 0;
    bool broken = false;
    long calls_before_destroy = 0;

    bool step(const char* name, const std::function<int()>& f, const std::function<int()>& again = nullptr) {
        if (broken) return false;
        int rc = f();
        if (rc == SIXDOF_OK) return true;
        const char* msg = sixdof_last_error(h);
        const std::string first = msg ? msg : "";
        if (!hip_fake::fired() || failed_steps || first.empty()) {
            complain(std::string(name) + " failed (status " + std::to_string(rc) + ") " + (first.empty() ? "without a message" : "with no fault of the test's behind it: " + first));
            return broken = true, false;
        }
        failed_steps++;
        rc = (again ? again : f)();
        if (rc == SIXDOF_OK) return true;
        msg = sixdof_last_error(h);
        complain(std::string(name) + " failed on the injected fault (" + first + ") and failed again without one (status " + std::to_string(rc) + "): " + (msg ? msg : ""));
        return broken = true, false;
    }

    bool edges(const std::vector<uint64_t>& from, const std::vector<uint64_t>& to) {
        if (!step("set_edges", [&] { return sixdof_set_edges(h, from.data(), to.data(), from.size()); })) return false;
        std::vector<uint32_t> src(8), dst(8);
        size_t n = 0;
        if (sixdof_get_edge_rows(h, src.data(), dst.data(), 8, &n) != SIXDOF_OK || n != from.size()) return complain("get_edge_rows after set_edges"), broken = true, false;
        for (size_t e = 0; e < n; e++) w.edge_rows.push_back(src[e]), w.edge_rows.push_back(dst[e]);
        return true;
    }

    void scenario() {
        const long calls0 = hip_fake::calls();
        sixdof_desc d{};
        d.struct_size = sizeof(d), d.integrator = SIXDOF_INTEGRATOR_RK4, d.dtype = SIXDOF_F64, d.simulation_time_step = 1.0 / 120.0, d.ticks_per_launch = 1;
        step("create", [&] { return sixdof_create(&d, &h); });
        auto cols = w.columns(false);
        auto bind = [&] { return sixdof_bind_columns(h, cols.data(), cols.size()); };
        auto upload = [&] { return sixdof_upload(h); };
        auto bind_upload = [&] { int rc = bind(); return rc != SIXDOF_OK ? rc : upload(); };
        step("bind_columns", bind, bind_upload);
        step("upload", upload);
        edges({1, 1, 4}, {2, 3, 5});
        sixdof_effector_op pair{};
        pair.kind = SIXDOF_EFF_EDGE_GRAVITY_NEWTON, pair.p[0] = 1.0;
        step("set_effectors", [&] { return sixdof_set_effectors(h, &pair, 1); });
        step("step (pair op)", [&] { return sixdof_step(h, 2, nullptr); });
        step("download", [&] { return sixdof_download(h, SIXDOF_COL_ALL); });
        step("download_async", [&] { return sixdof_download_async(h, SIXDOF_COL_ALL); });
        step("download_wait", [&] { return sixdof_download_wait(h); });
        const uint64_t extra_id = sixdof_component_id("extra"), pos_id = sixdof_component_id("world_pos");
        step("set_custom_pipe", [&] { return sixdof_set_custom_pipe(h, g_program, &extra_id, 1); });
        const uint64_t ffrom[3] = {2, 2, 7}, fto[3] = {1, 3, 8};
        step("set_fold_edges", [&] { return sixdof_set_fold_edges(h, 0, ffrom, fto, 3); });
        step("set_history", [&] { return sixdof_set_history(h, 4); });
        step("step (program, ring)", [&] { return sixdof_step(h, 3, nullptr); });
        if (h) sixdof_get_tick(h, &w.tick);
        w.hist_pos.assign(kN * 7, -1.0), w.hist_extra.assign(kN * 2, -1.0);
        step("history_read", [&] { return sixdof_history_read(h, pos_id, w.tick, w.hist_pos.data()); });
        step("history_read (program column)", [&] { return sixdof_history_read(h, extra_id, w.tick - 1, w.hist_extra.data()); });
        void* sdst[4];
        for (int k = 0; k < 4; k++) w.stream[k].assign(2 * kN * (k == 0 ? 7 : 6), -1.0), sdst[k] = w.stream[k].data();
        step("history_stream", [&] { return sixdof_history_stream(h, w.tick - 1, 2, sdst); });
        const uint64_t watch_ids[2] = {pos_id, extra_id}, watch_entities[2] = {3, 5};
        step("set_watch", [&] { return sixdof_set_watch(h, watch_ids, 2, watch_entities, 2); });
        for (int a = 0; a < 2; a++) {   // blocking, then asynchronous
            w.watch_pos[a].assign(2 * 2 * 7, -1.0), w.watch_extra[a].assign(2 * 2 * 2, -1.0);
            void* wdst[2] = {w.watch_pos[a].data(), w.watch_extra[a].data()};
            step(a ? "watch_read (async)" : "watch_read", [&] { return sixdof_watch_read(h, w.tick - 2, 2, 2, wdst, a ? SIXDOF_WATCH_ASYNC : 0u); });
        }
        step("download_wait (watch)", [&] { return sixdof_download_wait(h); });
        step("sync", [&] { return sixdof_sync(h); });
        cols = w.columns(true);   // the extra column three times as wide
        step("bind_columns (again)", bind, bind_upload);
        edges({6, 7}, {7, 6});
        step("set_history (again)", [&] { return sixdof_set_history(h, 2); });
        step("set_watch (clear)", [&] { return sixdof_set_watch(h, nullptr, 0, nullptr, 0); });
        w.flags.assign(kN, 0xff);
        step("count_nonfinite", [&] { return sixdof_count_nonfinite(h, &w.nonfinite, w.flags.data()); });
        calls_before_destroy = hip_fake::calls() - calls0;
        sixdof_destroy(h);
        h = nullptr;
    }
};

// what must hold after any run, with or without a fault
void check_clean(const std::string& run) {
    if (hip_fake::live_allocations() || hip_fake::live_streams() || hip_fake::live_events() || hip_fake::live_page_locks())
        complain(run + ": after sixdof_destroy " + std::to_string(hip_fake::live_allocations()) + " allocations, " + std::to_string(hip_fake::live_streams()) +
                 " streams, " + std::to_string(hip_fake::live_events()) + " events and " + std::to_string(hip_fake::live_page_locks()) + " page locks are alive");
}

// A handle with six columns bound and uploaded, for the named cases.
struct Bound {
    World w;
    sixdof_handle* h = nullptr;
    std::vector<sixdof_column> cols;
    Bound() {
        sixdof_desc d{};
        d.struct_size = sizeof(d), d.integrator = SIXDOF_INTEGRATOR_RK4, d.dtype = SIXDOF_F64, d.simulation_time_step = 1.0 / 120.0, d.ticks_per_launch = 1;
        cols = w.columns(false);
        if (sixdof_create(&d, &h) != SIXDOF_OK || sixdof_bind_columns(h, cols.data(), cols.size()) != SIXDOF_OK || sixdof_upload(h) != SIXDOF_OK)
            complain(std::string("named case: setup: ") + sixdof_last_error(h));
    }
    ~Bound() { sixdof_destroy(h); }
};

// Case 2: the copy lane recovers from a partial creation.  The first event of the lane cannot be created; the next
// sixdof_download_async must work.
void case_copy_lane() {
    Bound b;
    hip_fake::fail_after(2 * 5 + 1);   // the five snapshots (allocation, device copy) come first; then 10: the copy stream, 11: its first event
    if (sixdof_download_async(b.h, SIXDOF_COL_ALL) == SIXDOF_OK || !hip_fake::fired()) complain("copy lane: the injected fault did not fail download_async");
    hip_fake::fail_after(-1);
    if (sixdof_download_async(b.h, SIXDOF_COL_ALL) != SIXDOF_OK) complain(std::string("copy lane: download_async does not work on the retry: ") + sixdof_last_error(b.h));
    else if (sixdof_download_wait(b.h) != SIXDOF_OK) complain(std::string("copy lane: download_wait after the retry: ") + sixdof_last_error(b.h));
}

// Case 3: a failed sixdof_set_edges.  What sixdof_get_edge_rows reports and the tables the next step hands to the pair
// kernel (checked by the fake's launch stub: live, long enough, row_start[n] == n_edges) agree — on the old three edges.
void case_set_edges() {
    for (long fault : {0L, 2L}) {   // 0: the allocation of row_start; 2: the allocation of dst, with the new row_start already uploaded
        Bound b;
        const std::string name = "failed set_edges (fallible call " + std::to_string(fault) + ")";
        const uint64_t from[3] = {1, 1, 4}, to[3] = {2, 3, 5};
        sixdof_effector_op pair{};
        pair.kind = SIXDOF_EFF_EDGE_GRAVITY_NEWTON, pair.p[0] = 1.0;
        if (sixdof_set_edges(b.h, from, to, 3) != SIXDOF_OK || sixdof_set_effectors(b.h, &pair, 1) != SIXDOF_OK) complain(name + ": setup");
        hip_fake::fail_after(fault);
        if (sixdof_set_edges(b.h, from, to, 2) == SIXDOF_OK || !hip_fake::fired()) complain(name + ": the injected fault did not fail the call");
        hip_fake::fail_after(-1);
        size_t n = 0;
        uint32_t src[3], dst[3];
        const long before = hip_fake::violations();
        if (sixdof_get_edge_rows(b.h, src, dst, 3, &n) != SIXDOF_OK || n != 3 || src[2] != 3 || dst[2] != 4)
            complain(name + ": get_edge_rows no longer reports the three edges of the last successful call");
        if (sixdof_step(b.h, 1, nullptr) != SIXDOF_OK || hip_fake::violations() != before)
            complain(name + ": get_edge_rows reports " + std::to_string(n) + " edges, but the next step's tables disagree: " + sixdof_last_error(b.h));
    }
}

// Case 1: a failed re-bind.  The wider extra column cannot be allocated: the handle is unbound, nothing is freed twice
// (AddressSanitizer would say so at sixdof_destroy at the latest), and a later bind succeeds.
void case_rebind() {
    Bound b;
    b.cols = b.w.columns(true);
    hip_fake::fail_after(0);   // the five Body columns keep their device copies: the first call that can fail is the extra column's allocation
    if (sixdof_bind_columns(b.h, b.cols.data(), b.cols.size()) == SIXDOF_OK || !hip_fake::fired()) complain("failed re-bind: the injected fault did not fail the call");
    hip_fake::fail_after(-1);
    if (sixdof_upload(b.h) != SIXDOF_ERR_COMPONENT_NOT_FOUND) complain("failed re-bind: the handle still accepts an upload (it should be unbound)");
    if (sixdof_bind_columns(b.h, b.cols.data(), b.cols.size()) != SIXDOF_OK || sixdof_upload(b.h) != SIXDOF_OK)
        complain(std::string("failed re-bind: a later bind and upload fail: ") + sixdof_last_error(b.h));
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1) g_program = argv[1];
    case_copy_lane();
    check_clean("copy lane");
    case_set_edges();
    check_clean("failed set_edges");
    case_rebind();
    check_clean("failed re-bind");

    // the sweep, with everything completing at once and once more with every stream a queue that runs at forcing points only: a
    // fault in a deferred operation is then reported by the step that reaches it, and the reads are the same bytes
    long n_calls = 0, n_lazy = 0;
    uint64_t want = 0;
    for (int schedule : {int(hip_fake::kAtOnce), int(hip_fake::kMinimal)}) {
        const std::string mode = schedule == hip_fake::kAtOnce ? "" : std::string(hip_fake::schedule_name(schedule)) + ": ";
        hip_fake::set_schedule(schedule);
        hip_fake::fail_after(-1);
        Run clean;
        clean.scenario();
        check_clean(mode + "fault-free run");
        if (clean.broken || clean.failed_steps) return std::fprintf(stderr, "capi_lifecycle_test: the fault-free run failed\n"), 1;
        if (clean.w.nonfinite != 0) complain(mode + "fault-free run: count_nonfinite");
        (schedule == hip_fake::kAtOnce ? n_calls : n_lazy) = clean.calls_before_destroy;
        if (schedule == hip_fake::kAtOnce) want = clean.w.digest();
        else if (clean.w.digest() != want) complain(mode + "the fault-free run's reads differ from those with everything completing at once");
        for (long k = 0; k < clean.calls_before_destroy; k++) {
            const std::string run = mode + "fault at call " + std::to_string(k);
            Run r;
            hip_fake::fail_after(k);
            r.scenario();
            hip_fake::fail_after(-1);
            if (r.broken) continue;   // said so already
            if (r.failed_steps != 1) complain(run + ": no step reported it");
            if (r.w.digest() != want) complain(run + ": the reads after the retry differ from the fault-free run's");
            check_clean(run);
        }
    }
    hip_fake::set_schedule(hip_fake::kAtOnce);
    if (hip_fake::violations()) complain(std::to_string(hip_fake::violations()) + " violations reported by the fake runtime");
    if (g_failures) return std::fprintf(stderr, "capi_lifecycle_test: %d failures\n", g_failures), 1;
    std::printf("capi_lifecycle_test: ok (3 named cases; N = %ld fallible calls, each failed once; %ld more under the minimal schedule)\n", n_calls, n_lazy);
    return 0;
}
