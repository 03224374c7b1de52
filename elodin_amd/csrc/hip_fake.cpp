// hip_fake.cpp — a host-only stand-in for the HIP runtime, the kernel launchers and the AQL queue, so that the whole
// host layer (sixdof_capi.cpp) links and runs under AddressSanitizer without a GPU: `make capi_test`,
// capi_lifecycle_test.cpp.  Never part of the library.
//
// Device memory is calloc'd host memory, copies are memcpy, streams and events are small heap objects, everything
// completes at once.  The k-th FALLIBLE call (allocations, creations, copies, records, waits, synchronisations,
// launches) returns hipErrorOutOfMemory when armed; frees and destroys always succeed.  The fake keeps the live
// allocations, streams, events and page locks, and its launch stubs check that every table a launch is handed lies
// inside a live allocation of sufficient size.
//
// The ordered mode (hip_fake::set_schedule, order_host_test.cpp) drops "everything completes at once": every stream is a FIFO of
// deferred operations — copies, memsets, the launch stubs, event records and waits on events — with the arguments captured by value
// and the checks made when the operation runs.  Nothing runs before a forcing point (a synchronisation, a synchronous copy, a
// destruction).  What a forcing point runs, and in which order where the waits leave it free, is the schedule's choice:
//     kMinimal        only what the forcing point itself is entitled to: the stream or event named, and what it waits on
//     kComputeFirst   everything queued anywhere, the streams in order of their creation (a handle's compute stream runs ahead)
//     kCopyFirst      everything queued anywhere, the youngest stream first (the copy lane runs ahead as far as its waits allow)
// All three are orders a device may legally take.  The host destination of a queued device-to-host copy is filled with 0xFF bytes
// (a NaN in f32 and f64) when it is enqueued, so a host read before completion is a value; device destinations are left alone.
// hipFree of an allocation a queued operation names and hipHostUnregister of a range a queued copy touches are violations, and a
// freed allocation's address is not handed out again while anything is queued, so a late operation cannot pass its check by luck.
// An injected fault in a deferred operation surfaces at the forcing point that reaches it: that call fails, the operation stays
// queued, and the next forcing point runs it — nothing is lost, as for a wait that was interrupted.  In every mode a page lock
// keeps its extent: an overlapping registration is refused, and a copy whose host side straddles the edge of a lock is a violation.
// What the fake still does not know: device page mappings (an access inside a live allocation's slack is invisible), other
// processes, and the runtime's internal pools and staging buffers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../include/sixdof_hip.h"
#include "aql_chain.hpp"
#include "covariance_plan.hpp"
#include "envelope_plan.hpp"
#include "events_plan.hpp"
#include "norms_plan.hpp"
#include "dwell_plan.hpp"
#include "norm_events_plan.hpp"
#include "extremes_plan.hpp"
#include "history_plan.hpp"
#include "kernels.hpp"
#include "quantile_plan.hpp"

namespace hip_fake {

std::map<const char*, size_t> g_allocs;
std::set<void*> g_streams, g_events;
std::map<const char*, size_t> g_pins;   // page locks: start -> bytes
long g_calls = 0, g_fail_at = -1, g_violations = 0;
bool g_fired = false;

// ---- the ordered mode -------------------------------------------------------------------------------------------------
enum { kAtOnce = 0, kMinimal = 1, kComputeFirst = 2, kCopyFirst = 3 };
int g_schedule = kAtOnce;
bool g_running = false;   // a deferred operation is being run: what it calls of the runtime happens at once
struct Op {
    std::string what;
    std::function<hipError_t()> run;    // empty: an event record or a wait
    std::vector<const void*> dev;       // the device pointers it names
    const char* host = nullptr;         // the host side of a copy
    size_t host_bytes = 0;
    void* wait_stream = nullptr;        // a wait: that stream must have completed wait_pos operations
    uint64_t wait_pos = 0;
};
struct Queue {
    uint64_t order = 0;                 // of creation
    bool non_blocking = false;
    std::deque<Op> ops;
    uint64_t done = 0;
    uint64_t enqueued() const { return done + ops.size(); }
};
struct Record { void* stream = nullptr; uint64_t pos = 0; };
std::map<void*, Queue> g_queues;        // by stream
std::map<void*, Record> g_records;      // by event: its latest record
std::vector<void*> g_quarantine;        // freed while something was queued: given back once every queue is empty
uint64_t g_order = 0;

void fail_after(long n) { g_fail_at = n < 0 ? -1 : g_calls + n, g_fired = false; }   // the n-th fallible call from now fails (once); < 0: none
bool fired() { return g_fired; }
long calls() { return g_calls; }
long violations() { return g_violations; }
size_t live_allocations() { return g_allocs.size(); }
size_t live_streams() { return g_streams.size(); }
size_t live_events() { return g_events.size(); }
size_t live_page_locks() { return g_pins.size(); }
// whether any page lock intersects [p, p + bytes)
bool lock_intersects(const void* p, size_t bytes) {
    const char* lo = static_cast<const char*>(p);
    for (auto& kv : g_pins)
        if (kv.first < lo + bytes && lo < kv.first + kv.second) return true;
    return false;
}
size_t queued() {
    size_t n = 0;
    for (auto& kv : g_queues) n += kv.second.ops.size();
    return n;
}
const char* schedule_name(int schedule) {
    return schedule == kAtOnce ? "at-once" : schedule == kMinimal ? "minimal" : schedule == kComputeFirst ? "compute-first" : "copy-first";
}

static hipError_t fallible() {
    if (g_calls++ != g_fail_at) return hipSuccess;
    g_fired = true;
    return hipErrorOutOfMemory;
}
// [p, p + bytes) lies inside one live allocation
static bool live(const void* p, size_t bytes) {
    auto it = g_allocs.upper_bound(static_cast<const char*>(p));
    if (!p || it == g_allocs.begin()) return false;
    --it;
    return static_cast<const char*>(p) + bytes <= it->first + it->second;
}
static bool need(bool ok, const char* what) {
    if (!ok) std::fprintf(stderr, "hip_fake: a launch was handed a table that is not (wholly) a live allocation: %s\n", what), g_violations++;
    return ok;
}
static hipError_t launch(bool ok) {
    if (!g_running)   // a deferred operation was counted (and may have been failed) before it ran
        if (hipError_t e = fallible(); e != hipSuccess) return e;
    return ok ? hipSuccess : hipErrorInvalidValue;
}

static void flush_quarantine() {
    if (queued()) return;
    for (void* p : g_quarantine) std::free(p);
    g_quarantine.clear();
}
// Runs the operations of stream s until `upto` of them have completed, and before each wait what it waits on.  An injected fault
// leaves its operation queued and ends the drain; an operation that fails its own checks is dropped, and reported once the drain is done.
static hipError_t drain(void* s, uint64_t upto) {
    auto it = g_queues.find(s);
    if (it == g_queues.end()) return hipSuccess;   // destroyed, hence drained
    Queue& q = it->second;
    hipError_t first = hipSuccess;
    while (q.done < upto && !q.ops.empty()) {
        Op& op = q.ops.front();
        if (op.wait_stream)
            if (hipError_t e = drain(op.wait_stream, op.wait_pos); e != hipSuccess) return e;
        if (op.run) {
            if (hipError_t e = fallible(); e != hipSuccess) return e;
            g_running = true;
            const hipError_t e = op.run();
            g_running = false;
            if (e != hipSuccess && first == hipSuccess) first = e;
        }
        q.ops.pop_front();
        q.done++;
    }
    return first;
}
static hipError_t drain_all(bool youngest_first, bool blocking_only = false) {
    std::vector<std::pair<uint64_t, void*>> order;
    for (auto& kv : g_queues)
        if (!blocking_only || !kv.second.non_blocking) order.emplace_back(kv.second.order, kv.first);
    std::sort(order.begin(), order.end());
    if (youngest_first) std::reverse(order.begin(), order.end());
    hipError_t first = hipSuccess;
    for (auto& o : order) {
        auto it = g_queues.find(o.second);
        if (it == g_queues.end()) continue;
        const hipError_t e = drain(o.second, it->second.enqueued());
        if (e == hipErrorOutOfMemory) return e;
        if (e != hipSuccess && first == hipSuccess) first = e;
    }
    return first;
}
// A forcing point: stream s has to complete `upto` operations (s null: every stream everything).
static hipError_t force(void* s, uint64_t upto) {
    hipError_t e;
    if (g_schedule == kComputeFirst || g_schedule == kCopyFirst) e = drain_all(g_schedule == kCopyFirst);
    else e = s ? drain(s, upto) : drain_all(false);
    flush_quarantine();
    return e;
}
static bool deferring() { return g_schedule != kAtOnce && !g_running; }
static hipError_t defer(hipStream_t s, const char* what, std::vector<const void*> dev, std::function<hipError_t()> run, const void* host = nullptr, size_t host_bytes = 0) {
    auto it = g_queues.find(s);
    if (it == g_queues.end()) return need(false, (std::string(what) + " on a null or destroyed stream").c_str()), hipErrorInvalidHandle;
    Op op;
    op.what = what, op.run = std::move(run), op.dev = std::move(dev), op.host = static_cast<const char*>(host), op.host_bytes = host_bytes;
    it->second.ops.push_back(std::move(op));
    return hipSuccess;
}
// kAtOnce: everything completes at once (the default); otherwise one of the schedules above.  Whatever is queued runs first.
void set_schedule(int schedule) {
    (void)drain_all(false), (void)drain_all(false);   // twice: an armed fault may have ended the first pass
    flush_quarantine();
    g_schedule = schedule;
}

}  // namespace hip_fake
using namespace hip_fake;

// ---- the runtime ----------------------------------------------------------------------------------------------
const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : e == hipErrorOutOfMemory ? "out of memory (injected)" : "error"; }
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipGetDeviceCount(int* n) { return *n = 1, hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipMalloc(void** p, size_t bytes) {
    *p = nullptr;
    if (hipError_t e = fallible(); e != hipSuccess) return e;
    *p = std::calloc(bytes ? bytes : 1, 1);
    g_allocs[static_cast<const char*>(*p)] = bytes;
    return hipSuccess;
}
hipError_t hipFree(void* p) {
    if (!p) return hipSuccess;
    auto it = g_allocs.find(static_cast<const char*>(p));
    if (it == g_allocs.end()) {
        std::fprintf(stderr, "hip_fake: hipFree of %p, which is not a live allocation\n", p), g_violations++;
        std::free(p);   // a second free of the same pointer is AddressSanitizer's to report
        return hipSuccess;
    }
    // the real hipFree synchronises; the host layer must not lean on that
    for (auto& kv : g_queues)
        for (const Op& op : kv.second.ops)
            for (const void* d : op.dev)
                if (d >= it->first && d < it->first + (it->second ? it->second : 1))
                    std::fprintf(stderr, "hip_fake: hipFree of an allocation that a queued %s still names\n", op.what.c_str()), g_violations++;
    g_allocs.erase(it);
    if (queued()) g_quarantine.push_back(p);
    else std::free(p);
    return hipSuccess;
}
static hipError_t create(std::set<void*>& live_set, void** out) {
    *out = nullptr;
    if (hipError_t e = fallible(); e != hipSuccess) return e;
    live_set.insert(*out = std::malloc(8));
    return hipSuccess;
}
static hipError_t destroy(std::set<void*>& live_set, void* p) {
    if (!live_set.erase(p)) return std::fprintf(stderr, "hip_fake: destroy of %p, which is not live\n", p), g_violations++, hipErrorInvalidValue;
    std::free(p);
    return hipSuccess;
}
static hipError_t create_stream(hipStream_t* s, unsigned flags) {
    const hipError_t e = create(g_streams, reinterpret_cast<void**>(s));
    if (e == hipSuccess) g_queues[*s].order = g_order++, g_queues[*s].non_blocking = (flags & hipStreamNonBlocking) != 0;
    return e;
}
// a stream or event handed to record / wait / synchronise: null or destroyed is an error (the null stream is legal to query only)
static hipError_t use(bool ok) {
    if (hipError_t e = fallible(); e != hipSuccess) return e;
    if (!ok) std::fprintf(stderr, "hip_fake: null or destroyed stream / event\n"), g_violations++;
    return ok ? hipSuccess : hipErrorInvalidHandle;
}
hipError_t hipStreamCreate(hipStream_t* s) { return create_stream(s, 0); }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned flags) { return create_stream(s, flags); }
// destroying a stream or an event with work outstanding is legal: the work completes first
hipError_t hipStreamDestroy(hipStream_t s) {
    if (auto it = g_queues.find(s); it != g_queues.end()) {
        (void)drain(s, it->second.enqueued());
        g_queues.erase(s);
        flush_quarantine();
    }
    return destroy(g_streams, s);
}
hipError_t hipStreamSynchronize(hipStream_t s) {
    if (hipError_t e = use(g_streams.count(s)); e != hipSuccess) return e;
    return force(s, g_queues[s].enqueued());
}
hipError_t hipDeviceSynchronize(void) {
    if (hipError_t e = fallible(); e != hipSuccess) return e;
    return force(nullptr, 0);
}
hipError_t hipStreamQuery(hipStream_t s) {
    auto it = g_queues.find(s);
    return it != g_queues.end() && !it->second.ops.empty() ? hipErrorNotReady : hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) {
    if (hipError_t r = use(g_streams.count(s) && g_events.count(e)); r != hipSuccess) return r;
    if (!deferring()) return hipSuccess;
    auto rec = g_records.find(e);
    if (rec == g_records.end()) return hipSuccess;   // never recorded: nothing to wait for
    Op op;
    op.what = "wait", op.wait_stream = rec->second.stream, op.wait_pos = rec->second.pos;
    g_queues[s].ops.push_back(std::move(op));
    return hipSuccess;
}
hipError_t hipStreamBeginCapture(hipStream_t, hipStreamCaptureMode) { return hipErrorNotSupported; }
hipError_t hipStreamEndCapture(hipStream_t, hipGraph_t* g) { return *g = nullptr, hipErrorNotSupported; }
hipError_t hipGraphInstantiate(hipGraphExec_t*, hipGraph_t, hipGraphNode_t*, char*, size_t) { return hipErrorNotSupported; }
hipError_t hipGraphDestroy(hipGraph_t) { return hipSuccess; }
hipError_t hipGraphExecDestroy(hipGraphExec_t) { return hipSuccess; }
hipError_t hipGraphUpload(hipGraphExec_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t hipGraphLaunch(hipGraphExec_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t hipEventCreate(hipEvent_t* e) { return create(g_events, reinterpret_cast<void**>(e)); }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return create(g_events, reinterpret_cast<void**>(e)); }
hipError_t hipEventDestroy(hipEvent_t e) {
    if (auto rec = g_records.find(e); rec != g_records.end()) {
        (void)drain(rec->second.stream, rec->second.pos);
        g_records.erase(rec);
        flush_quarantine();
    }
    return destroy(g_events, e);
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
    if (hipError_t r = use(g_events.count(e) && g_streams.count(s)); r != hipSuccess) return r;
    if (!deferring()) return g_records.erase(e), hipSuccess;
    Op op;
    op.what = "record";
    Queue& q = g_queues[s];
    q.ops.push_back(std::move(op));
    g_records[e] = Record{s, q.enqueued()};
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e) {
    if (hipError_t r = use(g_events.count(e)); r != hipSuccess) return r;
    auto rec = g_records.find(e);
    return rec == g_records.end() ? hipSuccess : force(rec->second.stream, rec->second.pos);
}
hipError_t hipEventQuery(hipEvent_t e) {
    auto rec = g_records.find(e);
    if (rec == g_records.end()) return hipSuccess;
    auto q = g_queues.find(rec->second.stream);
    return q != g_queues.end() && q->second.done < rec->second.pos ? hipErrorNotReady : hipSuccess;
}
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { return *ms = 0.f, hipSuccess; }
hipError_t hipHostRegister(void* p, size_t bytes, unsigned) {
    if (!p || !bytes) return hipErrorInvalidValue;
    if (lock_intersects(p, bytes)) return hipErrorHostMemoryAlreadyRegistered;
    g_pins[static_cast<const char*>(p)] = bytes;
    return hipSuccess;
}
hipError_t hipHostUnregister(void* p) {
    auto it = g_pins.find(static_cast<const char*>(p));
    if (it == g_pins.end()) return hipErrorHostMemoryNotRegistered;
    for (auto& kv : g_queues)
        for (const Op& op : kv.second.ops)
            if (op.host && op.host < it->first + it->second && it->first < op.host + op.host_bytes)
                std::fprintf(stderr, "hip_fake: hipHostUnregister of a range that a queued %s still touches\n", op.what.c_str()), g_violations++;
    g_pins.erase(it);
    return hipSuccess;
}
// the host side of a copy lies wholly inside a page lock or touches none: what the runtime does with a partly locked range is unspecified
static void host_extent(const void* p, size_t bytes, const char* what) {
    const char* lo = static_cast<const char*>(p);
    for (auto& kv : g_pins)
        if (kv.first < lo + bytes && lo < kv.first + kv.second && !(kv.first <= lo && lo + bytes <= kv.first + kv.second))
            std::fprintf(stderr, "hip_fake: the host side of a %s of %zu bytes straddles the edge of a page lock of %zu bytes\n", what, bytes, kv.second), g_violations++;
}
// whichever side is device memory must be live; the other side is the caller's (AddressSanitizer watches the memcpy itself)
static hipError_t copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    if (!g_running)
        if (hipError_t e = fallible(); e != hipSuccess) return e;
    const bool dst_dev = kind == hipMemcpyHostToDevice || kind == hipMemcpyDeviceToDevice, src_dev = kind == hipMemcpyDeviceToHost || kind == hipMemcpyDeviceToDevice;
    if (!need(!dst_dev || live(dst, bytes), "copy destination") || !need(!src_dev || live(src, bytes), "copy source")) return hipErrorInvalidValue;
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}
static const char* copy_name(hipMemcpyKind kind) {
    return kind == hipMemcpyDeviceToHost ? "device-to-host copy" : kind == hipMemcpyHostToDevice ? "host-to-device copy" : "device-to-device copy";
}
static void copy_host_side(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    if (kind == hipMemcpyDeviceToHost) host_extent(dst, bytes, copy_name(kind));
    if (kind == hipMemcpyHostToDevice) host_extent(src, bytes, copy_name(kind));
}
// the synchronous form waits for the null stream, and with it for every blocking stream; then it runs at once
hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    copy_host_side(dst, src, bytes, kind);
    if (deferring()) {
        const hipError_t e = g_schedule == kMinimal ? drain_all(false, true) : force(nullptr, 0);
        flush_quarantine();
        if (e != hipSuccess) return e;
    }
    return copy(dst, src, bytes, kind);
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
    if (!need(g_streams.count(s), "copy on a null or destroyed stream")) return hipErrorInvalidHandle;
    copy_host_side(dst, src, bytes, kind);
    if (!deferring()) return copy(dst, src, bytes, kind);
    std::vector<const void*> dev;
    if (kind != hipMemcpyHostToDevice) dev.push_back(src);
    if (kind != hipMemcpyDeviceToHost) dev.push_back(dst);
    const void* host = kind == hipMemcpyDeviceToHost ? dst : kind == hipMemcpyHostToDevice ? src : nullptr;
    if (kind == hipMemcpyDeviceToHost) std::memset(dst, 0xFF, bytes);   // poison: a NaN in either width until the copy has run
    return defer(s, copy_name(kind), std::move(dev), [=] { return copy(dst, src, bytes, kind); }, host, host ? bytes : 0);
}
hipError_t hipMemsetAsync(void* dst, int v, size_t bytes, hipStream_t s) {
    if (deferring()) return defer(s, "memset", {dst}, [=] { return hipMemsetAsync(dst, v, bytes, s); });
    if (!g_running)
        if (hipError_t e = fallible(); e != hipSuccess) return e;
    if (!need(live(dst, bytes), "memset destination")) return hipErrorInvalidValue;
    std::memset(dst, v, bytes);
    return hipSuccess;
}

// ---- the launchers (kernels.hpp): no arithmetic, but every pointer a real kernel would follow is checked ---------
namespace sixdof {

static bool body_ok(const void* pos, const void* vel, const void* accel, const void* force, const void* inertia, size_t n, size_t es) {
    return need(live(pos, n * 7 * es), "world_pos") & need(live(vel, n * 6 * es), "world_vel") & need(live(accel, n * 6 * es), "world_accel") &
           need(live(force, n * 6 * es), "force") & need(live(inertia, n * 7 * es), "inertia");
}
static bool ops_ok(const DevOp* ops, uint32_t n_ops, size_t n, size_t es) {
    bool ok = true;
    for (uint32_t k = 0; k < n_ops; k++)
        if (ops[k].aux) ok &= need(live(ops[k].aux, n * (ops[k].aux_width ? ops[k].aux_width : 3) * es), "effector aux column");
    return ok;
}
static bool step_ok(const StepParams& p, int dtype) {
    const size_t n = p.n, es = dtype == 1 ? 4 : 8;
    bool ok = body_ok(p.pos, p.vel, p.accel, p.force, p.inertia, n, es) & ops_ok(p.ops, p.n_ops, n, es);
    if (p.hist_ring) {
        const size_t r = p.hist_ring;
        ok &= need(live(p.hist_pos, r * n * 7 * es), "hist_pos") & need(live(p.hist_vel, r * n * 6 * es), "hist_vel") &
              need(live(p.hist_accel, r * n * 6 * es), "hist_accel") & need(live(p.hist_force, r * n * 6 * es), "hist_force");
    }
    for (int k = 0; k < kMaxModelCols; k++) {
        if (p.model_cols[k]) ok &= need(live(p.model_cols[k], n * es), "program column");
        if (p.model_hist[k]) ok &= need(live(p.model_hist[k], p.hist_ring * n * es), "program column ring");
    }
    return ok;
}
static bool pair_ok(const PairParams& p) {
    const size_t n = p.n, u = sizeof(uint32_t), d = sizeof(double);
    bool ok = body_ok(p.pos, p.vel, p.accel, p.force, p.inertia, n, 8) & ops_ok(p.ops, p.n_ops, n, 8);
    if (n) ok &= need(live(p.pack, n * kPackWidth * d), "pack") & need(live(p.partial, n * p.partial_width * p.splits * d), "partial");
    if (n && p.pack_next) ok &= need(live(p.pack_next, n * kPackWidth * d), "pack_next");
    if (p.pair_kind != SIXDOF_EFF_ALLPAIRS_GRAVITY_SOFTENED) {
        ok &= need(live(p.row_start, (n + 1) * u), "row_start");
        if (ok) ok &= need(p.row_start[n] == p.n_edges, "row_start[n] != n_edges");
    }
    if (p.n_edges) ok &= need(live(p.dst, p.n_edges * u), "dst");
    if (p.n_hubs)
        ok &= need(live(p.hub_rows, p.n_hubs * u), "hub_rows") & need(live(p.hub_chunk_start, (p.n_hubs + 1) * u), "hub_chunk_start") &
              need(live(p.chunk_e0, p.n_hub_chunks * u), "chunk_e0") & need(live(p.chunk_row, p.n_hub_chunks * u), "chunk_row") &
              need(live(p.chunk_partial, size_t(p.n_hub_chunks) * kPartialWidth * d), "chunk_partial");
    return ok;
}

StepKernel select_step(const StepParams&, int, int) { return {}; }
// no arithmetic, but a recording launch leaves the (unchanged) Body columns in the ring slots of its ticks, as the kernel does:
// what reads the ring (history_read, watch_read, history_envelope) then sees what was uploaded before the step
hipError_t launch_step(const StepParams& p, int integrator, int dtype, hipStream_t s) {
    if (deferring()) return defer(s, "launch_step", {p.pos, p.vel, p.accel, p.force, p.hist_pos, p.hist_vel, p.hist_accel, p.hist_force}, [=] { return launch_step(p, integrator, dtype, s); });
    const bool ok = step_ok(p, dtype);
    if (ok && p.hist_ring && p.hist_pos) {
        const size_t es = dtype == 1 ? 4 : 8;
        const void* live_col[4] = {p.pos, p.vel, p.accel, p.force};
        void* rings[4] = {p.hist_pos, p.hist_vel, p.hist_accel, p.hist_force};
        for (uint32_t t = 0; t < p.n_ticks; t++)
            for (int k = 0; k < 4; k++) {
                const size_t block = size_t(p.n) * (k == 0 ? 7 : 6) * es;
                std::memcpy(static_cast<char*>(rings[k]) + (p.hist_slot0 + t) % p.hist_ring * block, live_col[k], block);
            }
    }
    return launch(ok);
}
uint32_t pair_splits_for(uint32_t) { return 1; }
static hipError_t launch_pair(const PairParams& p, hipStream_t s) {
    if (deferring()) return defer(s, "pair launch", {p.pos, p.vel, p.accel, p.force, p.pack, p.partial}, [=] { return launch(pair_ok(p)); });
    return launch(pair_ok(p));
}
hipError_t launch_pair_ticks(const PairParams& p, int, uint32_t n_ticks, hipStream_t s, uint64_t* launches) { return *launches += 1 + 2 * n_ticks, launch_pair(p, s); }
hipError_t launch_pair_small(const PairParams& p, int, uint32_t, hipStream_t s, uint64_t* launches) { return *launches += 1, launch_pair(p, s); }
hipError_t launch_apollo(const ApolloParams&, hipStream_t s) {
    if (deferring()) return defer(s, "launch_apollo", {}, [] { return launch(true); });
    return launch(true);
}

static hipError_t move_rows(char* dst, const char* src, const uint32_t* rows, uint32_t m, size_t row, bool gather) {
    if (!need(live(rows, m * sizeof(uint32_t)), "join rows")) return launch(false);
    for (uint32_t j = 0; j < m; j++) {
        char* to = gather ? dst + j * row : dst + rows[j] * row;
        const char* from = gather ? src + rows[j] * row : src + j * row;
        if (!need(live(to, row) && live(from, row), "joined column")) return launch(false);
        std::memcpy(to, from, row);
    }
    return launch(true);
}
hipError_t launch_gather_rows(void* dst, const void* src, const uint32_t* rows, uint32_t m, uint32_t w, size_t elem, hipStream_t s) {
    if (deferring()) return defer(s, "gather_rows", {dst, src, rows}, [=] { return launch_gather_rows(dst, src, rows, m, w, elem, s); });
    return move_rows(static_cast<char*>(dst), static_cast<const char*>(src), rows, m, w * elem, true);
}
hipError_t launch_scatter_rows(void* dst, const void* src, const uint32_t* rows, uint32_t m, uint32_t w, size_t elem, hipStream_t s) {
    if (deferring()) return defer(s, "scatter_rows", {dst, src, rows}, [=] { return launch_scatter_rows(dst, src, rows, m, w, elem, s); });
    return move_rows(static_cast<char*>(dst), static_cast<const char*>(src), rows, m, w * elem, false);
}
// the gather itself (join_kernels.hip), so that watch reads return what the ring holds
hipError_t launch_history_gather(const HistoryGatherArgs& a, uint32_t n_components, void* out, const uint32_t* rows, uint64_t m, uint64_t n,
                                 uint64_t first_tick, uint64_t n_samples, uint64_t every, uint64_t ring, size_t elem, hipStream_t s) {
    if (deferring()) {
        std::vector<const void*> dev{out, rows};
        for (uint32_t c = 0; c < n_components; c++) dev.push_back(a.c[c].ring);
        return defer(s, "history_gather", std::move(dev), [=] { return launch_history_gather(a, n_components, out, rows, m, n, first_tick, n_samples, every, ring, elem, s); });
    }
    if (!need(live(rows, m * sizeof(uint32_t)), "watch rows")) return launch(false);
    for (uint32_t c = 0; c < n_components; c++) {
        const size_t row = a.c[c].w * elem;
        for (uint64_t e = 0; e < m; e++)
            for (uint64_t j = 0; j < n_samples; j++) {
                const char* from = static_cast<const char*>(a.c[c].ring) + (((first_tick + j * every - 1) % ring) * n + rows[e]) * row;
                char* to = static_cast<char*>(out) + a.c[c].out_offset * elem + (e * n_samples + j) * row;
                if (!need(live(from, row) && live(to, row), "ring or watch staging")) return launch(false);
                std::memcpy(to, from, row);
            }
    }
    return launch(true);
}
// The walk both reduction twins make over a launch: every component, every sample of the chunk.  The component's `units` scratch
// units of one sample fit the stride; the sample's block in the ring and its [period][planes][w] block in the staging buffer are
// live, and go to tick(d, j, src, to) — the arithmetic of one tick, all that differs between the twins.
template <class Units, class Tick>
static bool ring_bin_walk(const char* who, const RingBinArgs& a, uint32_t n_components, double* out, uint64_t planes, uint64_t stride, uint64_t n,
                          uint32_t period, uint64_t first_tick, uint64_t sample0, uint64_t n_samples, uint64_t every, uint64_t ring, size_t elem,
                          Units units, Tick tick) {
    const std::string scratch = std::string(who) + " scratch of one sample", blocks = std::string("ring or ") + who + " staging";
    for (uint32_t k = 0; k < n_components; k++) {
        const RingBinDesc& d = a.c[k];
        if (!envelope_supported(d.w, period)) return false;
        if (!need(d.scratch_offset + units(d) <= stride, scratch.c_str())) return false;
        const uint64_t total = n * d.w;
        for (uint64_t j = 0; j < n_samples; j++) {
            const char* src = static_cast<const char*>(d.ring) + sample_slot(first_tick, sample0 + j, every, ring) * total * elem;
            double* to = out + d.out_offset + (sample0 + j) * period * planes * d.w;
            if (!need(live(src, total * elem) && live(to, size_t(period) * planes * d.w * sizeof(double)), blocks.c_str())) return false;
            tick(d, j, src, to);
        }
    }
    return true;
}
// the reduction itself (envelope_kernels.hip), serially: envelope_plan.hpp's arithmetic in the kernels' geometry and merge order
hipError_t launch_history_envelope(const RingBinArgs& a, uint32_t n_components, double* out, void* partial, uint64_t partial_stride, uint64_t n,
                                   uint32_t period, uint64_t first_tick, uint64_t sample0, uint64_t n_samples, uint64_t every, uint64_t ring,
                                   size_t elem, hipStream_t s) {
    if (deferring()) {
        std::vector<const void*> dev{out, partial};
        for (uint32_t c = 0; c < n_components && c < kRingBinMaxComponents; c++) dev.push_back(a.c[c].ring);
        return defer(s, "history_envelope", std::move(dev), [=] {
            return launch_history_envelope(a, n_components, out, partial, partial_stride, n, period, first_tick, sample0, n_samples, every, ring, elem, s);
        });
    }
    if (!envelope_launch_ok(n_components, kRingBinMaxComponents, n_samples, period)) return launch(false);
    EnvelopePartial* part = static_cast<EnvelopePartial*>(partial);
    if (!need(live(part, n_samples * partial_stride * sizeof(EnvelopePartial)), "envelope partial records")) return launch(false);
    if (n == 0) return launch(true);
    std::vector<EnvelopePartial> rec(kEnvelopeThreads);
    auto records = [&](const RingBinDesc& d) {
        const EnvelopeGeom g = envelope_geom(n, d.w, period);
        return uint64_t(g.blocks) * g.bins;
    };
    return launch(ring_bin_walk("envelope", a, n_components, out, kEnvelopeStats, partial_stride, n, period, first_tick, sample0, n_samples, every, ring, elem, records,
                                [&](const RingBinDesc& d, uint64_t j, const char* src, double* to) {
        const EnvelopeGeom g = envelope_geom(n, d.w, period);
        const uint64_t total = n * d.w;
        EnvelopePartial* mine = part + j * partial_stride + d.scratch_offset;
        for (uint32_t b = 0; b < g.blocks; b++) {                       // stage 1
            for (uint32_t t = 0; t < g.tile; t++) {
                EnvelopePartial acc = envelope_empty();
                for (uint64_t i = uint64_t(b) * g.tile + t; i < total; i += uint64_t(g.blocks) * g.tile) {
                    double x;
                    if (elem == 8) std::memcpy(&x, src + i * 8, 8);
                    else { float f; std::memcpy(&f, src + i * 4, 4); x = f; }
                    envelope_accumulate(acc, x);
                }
                rec[t] = acc;
            }
            for (uint32_t bin = 0; bin < g.bins; bin++) {
                envelope_tree_fold(&rec[bin], g.per_bin, g.bins);
                mine[uint64_t(b) * g.bins + bin] = rec[bin];
            }
        }
        for (uint32_t bin = 0; bin < g.bins; bin++) {                   // stage 2
            EnvelopePartial r = mine[bin];
            for (uint32_t b = 1; b < g.blocks; b++) r = envelope_merge(r, mine[uint64_t(b) * g.bins + bin]);
            envelope_emit(r, to + uint64_t(bin / d.w) * kEnvelopeStats * d.w + bin % d.w, d.w);
        }
    }));
}
// the joint reduction itself (covariance_kernels.hip), serially: covariance_plan.hpp's arithmetic in the kernels' geometry and
// merge order, through the launch's own scratch in the kernels' [block][field][period] layout
template <int K>
static bool covariance_walk(const CovarianceArgs& a, double* out, double* part, uint64_t partial_stride, uint64_t n, uint32_t period, uint64_t first_tick,
                            uint64_t sample0, uint64_t n_samples, uint64_t every, uint64_t ring, size_t elem) {
    constexpr uint32_t F = covariance_fields(K);
    const CovarianceGeom g = covariance_geom(n, period);
    if (!need(covariance_scratch_doubles(g, K, period) <= partial_stride, "covariance scratch of one sample")) return false;
    std::vector<CovarianceRecord<K>> rec(kCovarianceThreads);
    for (uint64_t j = 0; j < n_samples; j++) {
        const uint64_t slot = sample_slot(first_tick, sample0 + j, every, ring);
        const char* src[K];
        for (int c = 0; c < K; c++) {
            if (!need(a.c[c].element < a.c[c].w, "covariance channel element")) return false;
            src[c] = static_cast<const char*>(a.c[c].ring) + slot * n * a.c[c].w * elem;
            if (!need(live(src[c], n * a.c[c].w * elem), "ring block of a covariance channel")) return false;
        }
        double* mine = part + j * partial_stride;
        double* to = out + (sample0 + j) * period * F;
        if (!need(live(to, size_t(period) * F * sizeof(double)), "covariance staging")) return false;
        for (uint32_t b = 0; b < g.blocks; b++) {                       // stage 1
            for (uint32_t t = 0; t < g.tile; t++) {
                CovarianceRecord<K> acc = covariance_empty<K>();
                for (uint64_t row = uint64_t(b) * g.tile + t; row < n; row += uint64_t(g.blocks) * g.tile) {
                    double x[K];
                    for (int c = 0; c < K; c++) {
                        const char* at = src[c] + (row * a.c[c].w + a.c[c].element) * elem;
                        if (elem == 8) std::memcpy(&x[c], at, 8);
                        else { float f; std::memcpy(&f, at, 4); x[c] = f; }
                    }
                    covariance_accumulate<K>(acc, x);
                }
                rec[t] = acc;
            }
            for (uint32_t grp = 0; grp < period; grp++) {
                covariance_tree_fold<K>(&rec[grp], g.per_group, period);
                for (uint32_t f = 0; f < F; f++) mine[(uint64_t(b) * F + f) * period + grp] = covariance_field(rec[grp], int(f));
            }
        }
        for (uint32_t grp = 0; grp < period; grp++) {                   // stage 2
            CovarianceRecord<K> r = covariance_empty<K>();
            for (uint32_t b = 0; b < g.blocks; b++) {
                CovarianceRecord<K> o;
                for (uint32_t f = 0; f < F; f++) covariance_field(o, int(f)) = mine[(uint64_t(b) * F + f) * period + grp];
                r = b == 0 ? o : covariance_merge<K>(r, o);
            }
            covariance_emit<K>(r, to + uint64_t(grp) * F);
        }
    }
    return true;
}
hipError_t launch_history_covariance(const CovarianceArgs& a, uint32_t k, double* out, void* partial, uint64_t partial_stride, uint64_t n, uint32_t period,
                                     uint64_t first_tick, uint64_t sample0, uint64_t n_samples, uint64_t every, uint64_t ring, size_t elem, hipStream_t s) {
    if (deferring()) {
        std::vector<const void*> dev{out, partial};
        for (uint32_t c = 0; c < k && c < kCovarianceArgChannels; c++) dev.push_back(a.c[c].ring);
        return defer(s, "history_covariance", std::move(dev), [=] {
            return launch_history_covariance(a, k, out, partial, partial_stride, n, period, first_tick, sample0, n_samples, every, ring, elem, s);
        });
    }
    if (!covariance_launch_ok(k, n_samples, period)) return launch(false);
    double* part = static_cast<double*>(partial);
    if (!need(live(part, n_samples * partial_stride * sizeof(double)), "covariance partial records")) return launch(false);
    if (n == 0) return launch(true);
    switch (k) {
    case 2: return launch(covariance_walk<2>(a, out, part, partial_stride, n, period, first_tick, sample0, n_samples, every, ring, elem));
    case 3: return launch(covariance_walk<3>(a, out, part, partial_stride, n, period, first_tick, sample0, n_samples, every, ring, elem));
    case 4: return launch(covariance_walk<4>(a, out, part, partial_stride, n, period, first_tick, sample0, n_samples, every, ring, elem));
    case 5: return launch(covariance_walk<5>(a, out, part, partial_stride, n, period, first_tick, sample0, n_samples, every, ring, elem));
    default: return launch(covariance_walk<6>(a, out, part, partial_stride, n, period, first_tick, sample0, n_samples, every, ring, elem));
    }
}
// the selection itself (quantile_kernels.hip), serially: quantile_plan.hpp's keys, scan step and lo -> hi rule, pass by pass in the
// launch's own scratch (one sample's slots at a time: the histograms and states of a bin are where the kernels keep them)
template <class E>
static void quantiles_of_tick(const char* src, uint64_t n, uint32_t w, uint32_t period, const QuantileRanks& rk, uint32_t* hist, QuantileSlot* state,
                              double* to) {
    using B = QuantileBits<E>;
    const QuantileGeom g = quantile_geom(n, w, period, rk.count);
    const uint32_t R = rk.count;
    std::vector<uint64_t> keys;
    for (uint32_t bin = 0; bin < g.bins; bin++) {
        keys.clear();
        for (uint64_t row = 0; row < g.rows; row++) {
            E x;
            std::memcpy(&x, src + (row * g.bins + bin) * sizeof(E), sizeof(E));
            if (B::finite(B::raw(x))) keys.push_back(B::key(B::raw(x)));
        }
        uint32_t* h = hist + uint64_t(bin) * R * kQuantileDigits;
        QuantileSlot* st = state + uint64_t(bin) * R;
        uint64_t prefix[kQuantileMaxRanks] = {};
        for (uint32_t pass = 0; pass < quantile_passes(B::bits); pass++) {
            std::memset(h, 0, size_t(R) * kQuantileDigits * sizeof(uint32_t));
            for (uint32_t r = 0; r < R; r++) prefix[r] = pass == 0 ? 0 : st[r].prefix;
            const uint64_t mask = quantile_prefix_mask(B::bits, pass);
            for (uint32_t r = 0; r < R; r++)
                if (quantile_alias(prefix, r) == r && (pass == 0 || !(st[r].flags & kQuantileEmpty)))
                    for (uint64_t key : keys)
                        if ((key & mask) == prefix[r]) h[r * kQuantileDigits + quantile_digit(key, quantile_shift(B::bits, pass))]++;
            for (uint32_t r = 0; r < R; r++) quantile_advance(st[r], h + quantile_alias(prefix, r) * kQuantileDigits, B::bits, pass, rk.num[r], rk.den);
        }
        for (uint32_t r = 0; r < R; r++) {
            uint64_t next = ~uint64_t(0);
            if (st[r].flags & kQuantileNeedNext)
                for (uint64_t key : keys)
                    if (key > st[r].prefix && key < next) next = key;
            quantile_emit<E>(st[r], next, r, to + uint64_t(bin / w) * (1 + 2 * R) * w + bin % w, w);
        }
    }
}
hipError_t launch_history_quantiles(const RingBinArgs& a, uint32_t n_components, const QuantileRanks& ranks, double* out, void* hist, void* state,
                                    uint64_t slot_stride, uint64_t n, uint32_t period, uint64_t first_tick, uint64_t sample0, uint64_t n_samples,
                                    uint64_t every, uint64_t ring, size_t elem, hipStream_t s) {
    if (deferring()) {
        std::vector<const void*> dev{out, hist, state};
        for (uint32_t c = 0; c < n_components && c < kRingBinMaxComponents; c++) dev.push_back(a.c[c].ring);
        return defer(s, "history_quantiles", std::move(dev), [=] {
            return launch_history_quantiles(a, n_components, ranks, out, hist, state, slot_stride, n, period, first_tick, sample0, n_samples, every, ring, elem, s);
        });
    }
    if (!quantile_launch_ok(n_components, kRingBinMaxComponents, ranks, n, n_samples, period)) return launch(false);
    if (n_samples == 0 || n == 0) return launch(true);
    // the clears the real launcher enqueues between the passes: the first of them stands for all, fallible like them
    if (hipError_t e = hipMemsetAsync(hist, 0, n_samples * slot_stride * kQuantileDigits * sizeof(uint32_t), s); e != hipSuccess) return e;
    if (!need(live(state, n_samples * slot_stride * sizeof(QuantileSlot)), "quantile slot states")) return launch(false);
    return launch(ring_bin_walk("quantile", a, n_components, out, 1 + 2 * uint64_t(ranks.count), slot_stride, n, period, first_tick, sample0, n_samples, every, ring, elem,
                                [&](const RingBinDesc& d) { return uint64_t(period) * d.w * ranks.count; },
                                [&](const RingBinDesc& d, uint64_t j, const char* src, double* to) {
        uint32_t* h = static_cast<uint32_t*>(hist) + (j * slot_stride + d.scratch_offset) * kQuantileDigits;
        QuantileSlot* st = static_cast<QuantileSlot*>(state) + j * slot_stride + d.scratch_offset;
        if (elem == 8) quantiles_of_tick<double>(src, n, d.w, period, ranks, h, st, to);
        else quantiles_of_tick<float>(src, n, d.w, period, ranks, h, st, to);
    }));
}
// ---- the scans over time: the walk and the merge themselves (extremes_, events_, norms_, norm_events_ and dwell_kernels.hip), serially ----
// The two stages of a scan launch in the kernels' segmentation (time_scan.hpp) for `units` units: walk(unit, lo, hi, start) -> record
// is the kernel's own walk over the samples [lo, hi); slot(segment, unit) is the unit's record in scratch, its fields `stride`
// apart — with more than one segment every (segment, unit) record goes through the launch's scratch, as on the device.  Record,
// rule and accumulator come with `acc`, one of the two below.
template <class Acc, class Walk, class Slot>
static void scan_stages(const Acc& acc, uint64_t units, uint64_t stride, uint32_t segments, bool merge_into, uint64_t n_samples, Walk walk, Slot slot) {
    using Record = typename Acc::Record;
    const bool resume = segments == 1 && merge_into;
    for (uint32_t seg = 0; seg < segments; seg++) {                        // stage 1
        const uint64_t lo = scan_segment_start(n_samples, segments, seg), hi = scan_segment_start(n_samples, segments, seg + 1);
        for (uint64_t u = 0; u < units; u++) {
            Record r = walk(u, lo, hi, resume && Acc::kWalksOn ? acc.held(u) : Acc::empty());
            if (segments > 1) {
                Acc::store(r, slot(seg, u), stride);
                continue;
            }
            if (resume && !Acc::kWalksOn) r = Acc::merge(acc.held(u), r);
            acc.emit(r, u);
        }
    }
    for (uint64_t u = 0; segments > 1 && u < units; u++) {                 // stage 2
        Record r = merge_into ? acc.held(u) : Acc::empty();
        for (uint32_t s = 0; s < segments; s++) r = Acc::merge(r, Acc::load(slot(s, u), stride));
        acc.emit(r, u);
    }
}
// The accumulator in the output planes, under extremes_plan.hpp's rule (the extremes, the norms): at(unit) is the unit's first
// plane, the planes of E `stride` apart.  A continuing one-segment walk starts empty and is merged behind what the planes hold.
template <class E, class At>
struct PlanesAcc {
    using Record = ExtremesRecord;
    static constexpr bool kWalksOn = false;
    uint64_t stride;
    At at;
    static Record empty() { return extremes_empty(); }
    static Record merge(const Record& earlier, const Record& later) { return extremes_merge(earlier, later); }
    static void store(const Record& r, uint64_t* base, uint64_t s) { extremes_store(r, base, s); }
    static Record load(const uint64_t* base, uint64_t s) { return extremes_load(base, s); }
    Record held(uint64_t u) const { return extremes_absorb<E>(at(u), stride); }
    void emit(const Record& r, uint64_t u) const { extremes_emit<E>(r, at(u), stride); }
};
template <class E, class At>
static PlanesAcc<E, At> planes_acc(uint64_t stride, At at) { return {stride, at}; }
// The accumulator in the output planes, under dwell_plan.hpp's rule (the dwell): at(unit) is the unit's first plane, the twelve
// planes `stride` apart.  A continuing one-segment walk starts empty and is merged behind what the planes hold.
template <class At>
struct DwellPlanesAcc {
    using Record = DwellRecord;
    static constexpr bool kWalksOn = false;
    uint64_t stride;
    At at;
    static Record empty() { return dwell_empty(); }
    static Record merge(const Record& earlier, const Record& later) { return dwell_merge(earlier, later); }
    static void store(const Record& r, uint64_t* base, uint64_t s) { dwell_store(r, base, s); }
    static Record load(const uint64_t* base, uint64_t s) { return dwell_load(base, s); }
    Record held(uint64_t u) const { return dwell_absorb(at(u), stride); }
    void emit(const Record& r, uint64_t u) const { dwell_emit(r, at(u), stride); }
};
template <class At>
static DwellPlanesAcc<At> dwell_planes_acc(uint64_t stride, At at) { return {stride, at}; }
// The accumulator in a record buffer, under events_plan.hpp's rule (the events, the norm events): mine(unit) is the unit's record,
// at(unit) its first output plane of E, both `runs` apart.  A continuing one-segment walk starts FROM the record, as the kernels do.
template <class E, class Mine, class At>
struct RecordsAcc {
    using Record = EventsRecord;
    static constexpr bool kWalksOn = true;
    uint64_t runs;
    uint32_t mode;
    Mine mine;
    At at;
    static Record empty() { return events_empty(); }
    static Record merge(const Record& earlier, const Record& later) { return events_merge(earlier, later); }
    static void store(const Record& r, uint64_t* base, uint64_t s) { events_store(r, base, s); }
    static Record load(const uint64_t* base, uint64_t s) { return events_load(base, s); }
    Record held(uint64_t u) const { return events_load(mine(u), runs); }
    void emit(const Record& r, uint64_t u) const { events_store(r, mine(u), runs), events_emit<E>(r, mode, at(u), runs); }
};
template <class E, class Mine, class At>
static RecordsAcc<E, Mine, At> records_acc(uint64_t runs, uint32_t mode, Mine mine, At at) { return {runs, mode, mine, at}; }
// f(E{}) for the ring's element type
template <class F>
static void with_elem(size_t elem, F f) {
    if (elem == 8) f(double{});
    else f(float{});
}
// The deferred form of a scan launch: `dev` and what rings(item, dev) adds for each of its items is the device memory it names.
template <class Rings, class Run>
static hipError_t defer_scan(hipStream_t s, const char* what, std::vector<const void*> dev, uint32_t items, uint32_t max_items, Rings rings, Run run) {
    for (uint32_t c = 0; c < items && c < max_items; c++) rings(c, dev);
    return defer(s, what, std::move(dev), run);
}
static void probe_rings(const NormsProbe& p, std::vector<const void*>& dev) {
    dev.push_back(p.ring_a);
    if (p.flags & kNormMinus) dev.push_back(p.ring_b);
}
static bool probe_live(const NormsProbe& p, uint64_t ring, uint64_t n, size_t elem) {
    return live(p.ring_a, ring * n * p.w_a * elem) && (!(p.flags & kNormMinus) || live(p.ring_b, ring * n * p.w_b * elem));
}
// extremes_plan.hpp's rule over the kernels' own loop (time_scan.hpp: scan_walk); a unit is one element of a row
hipError_t launch_history_extremes(const RingBinArgs& a, uint32_t n_components, double* out, void* scratch, uint64_t scratch_stride, uint32_t segments,
                                   bool merge_into, uint64_t n, uint64_t first_tick, uint64_t n_samples, uint64_t every, uint64_t ring, size_t elem,
                                   hipStream_t s) {
    if (deferring())
        return defer_scan(s, "history_extremes", {out, scratch}, n_components, kRingBinMaxComponents, [&](uint32_t c, auto& dev) { dev.push_back(a.c[c].ring); }, [=] {
            return launch_history_extremes(a, n_components, out, scratch, scratch_stride, segments, merge_into, n, first_tick, n_samples, every, ring, elem, s);
        });
    uint32_t widths[kRingBinMaxComponents] = {};
    for (uint32_t k = 0; k < n_components && k < kRingBinMaxComponents; k++) widths[k] = a.c[k].w;
    if (!extremes_launch_ok(n_components, kRingBinMaxComponents, widths, n, first_tick, n_samples, every, segments) || ring == 0) return launch(false);
    if (n == 0) return launch(true);
    if (segments > 1 && !need(live(scratch, scan_scratch_bytes(segments, scratch_stride, kExtremesFields)), "extremes scratch records")) return launch(false);
    for (uint32_t k = 0; k < n_components; k++) {
        const RingBinDesc& d = a.c[k];
        const uint64_t total = n * d.w;
        if (!need(segments == 1 || d.scratch_offset + total <= scratch_stride, "extremes scratch of one segment")) return launch(false);
        if (!need(live(d.ring, ring * total * elem) && live(out + d.out_offset, kExtremesPlanes * total * sizeof(double)), "ring or extremes staging"))
            return launch(false);
        with_elem(elem, [&](auto e) {
            using E = decltype(e);
            scan_stages(planes_acc<E>(total, [&](uint64_t i) { return out + d.out_offset + i; }), total, scratch_stride, segments, merge_into, n_samples,
                        [&](uint64_t i, uint64_t lo, uint64_t hi, const ExtremesRecord& start) {
                            return scan_walk(start, ExtremesRule{}, static_cast<const E*>(d.ring) + i, total, lo, hi, first_tick, every, ring);
                        },
                        [&](uint32_t seg, uint64_t i) { return static_cast<uint64_t*>(scratch) + uint64_t(seg) * kExtremesFields * scratch_stride + d.scratch_offset + i; });
        });
    }
    return launch(true);
}
// events_plan.hpp's rule over scan_walk, whose loop the kernel writes out; a unit is one run of a trigger.  The capture follows.
hipError_t launch_history_events(const EventsArgs& a, uint32_t n_triggers, void* rec, double* out, void* scratch, uint32_t segments, bool merge_into, uint64_t n,
                                 uint32_t period, uint64_t first_tick, uint64_t n_samples, uint64_t every, uint64_t ring, size_t elem, hipStream_t s) {
    if (deferring())
        return defer_scan(s, "history_events", {rec, out, scratch}, n_triggers, kEventsMaxTriggers, [&](uint32_t c, auto& dev) { dev.push_back(a.t[c].ring); }, [=] {
            return launch_history_events(a, n_triggers, rec, out, scratch, segments, merge_into, n, period, first_tick, n_samples, every, ring, elem, s);
        });
    if (!events_launch_ok(a, n_triggers, n, period, first_tick, n_samples, every, segments) || ring == 0) return launch(false);
    if (n == 0) return launch(true);
    const uint64_t runs = n / period, units = runs * n_triggers;
    if (segments > 1 && !need(live(scratch, scan_scratch_bytes(segments, units, kEventsFields)), "events scratch records")) return launch(false);
    if (!need(live(rec, events_record_bytes(units)) && live(out, units * kEventsPlanes * sizeof(double)), "events records or staging")) return launch(false);
    for (uint32_t k = 0; k < n_triggers; k++) {
        const EventsTrigger& t = a.t[k];
        if (!need(live(t.ring, ring * n * t.w * elem), "ring of a trigger")) return launch(false);
        with_elem(elem, [&](auto e) {
            using E = decltype(e);
            scan_stages(records_acc<E>(runs, t.mode, [&](uint64_t run) { return static_cast<uint64_t*>(rec) + uint64_t(k) * kEventsFields * runs + run; },
                                       [&](uint64_t run) { return out + uint64_t(k) * kEventsPlanes * runs + run; }),
                        runs, runs, segments, merge_into, n_samples,
                        [&](uint64_t run, uint64_t lo, uint64_t hi, const EventsRecord& start) {
                            return scan_walk(start, EventsRule{t.level, t.op, t.mode}, static_cast<const E*>(t.ring) + (run * period + t.group) * t.w + t.element, n * t.w,
                                             lo, hi, first_tick, every, ring);
                        },
                        [&](uint32_t seg, uint64_t run) { return static_cast<uint64_t*>(scratch) + (uint64_t(seg) * n_triggers + k) * kEventsFields * runs + run; });
        });
    }
    return launch(true);
}
hipError_t launch_events_capture(const EventsArgs& a, uint32_t n_triggers, const RingBinArgs& c, uint32_t n_captures, const void* rec, double* out, bool merge_into,
                                 uint64_t n, uint32_t period, uint64_t first_tick, uint64_t n_samples, uint64_t every, uint64_t ring, size_t elem, hipStream_t s) {
    if (deferring()) {
        std::vector<const void*> dev{rec, out};
        for (uint32_t k = 0; k < n_captures && k < kRingBinMaxComponents; k++) dev.push_back(c.c[k].ring);
        return defer(s, "events_capture", std::move(dev), [=] {
            return launch_events_capture(a, n_triggers, c, n_captures, rec, out, merge_into, n, period, first_tick, n_samples, every, ring, elem, s);
        });
    }
    uint32_t widths[kRingBinMaxComponents] = {};
    for (uint32_t k = 0; k < n_captures && k < kRingBinMaxComponents; k++) widths[k] = c.c[k].w;
    if (!events_capture_ok(a, n_triggers, n_captures, kRingBinMaxComponents, widths, n, period, first_tick, n_samples, every) || ring == 0) return launch(false);
    if (n == 0) return launch(true);
    const uint64_t runs = n / period, last = first_tick + (n_samples - 1) * every;
    const uint64_t* r = static_cast<const uint64_t*>(rec);
    if (!need(live(rec, events_record_bytes(runs * n_triggers)), "events records")) return launch(false);
    for (uint32_t k = 0; k < n_captures; k++) {
        const RingBinDesc& d = c.c[k];
        const uint64_t total = n * d.w;
        if (!need(live(d.ring, ring * total * elem) && live(out + d.out_offset, n_triggers * total * sizeof(double)), "ring or capture staging")) return launch(false);
        for (uint32_t trig = 0; trig < n_triggers; trig++)
            for (uint64_t i = 0; i < total; i++) {
                const uint64_t tick = events_stored_tick(r + uint64_t(trig) * kEventsFields * runs + i / d.w / period, runs, a.t[trig].mode);
                double* o = out + d.out_offset + uint64_t(trig) * total + i;
                if (events_tick_sampled(tick, first_tick, last, every)) {
                    const char* from = static_cast<const char*>(d.ring) + (history_slot(tick, ring) * total + i) * elem;
                    if (elem == 8) std::memcpy(o, from, 8);
                    else { float f; std::memcpy(&f, from, 4); *o = f; }
                } else if (!merge_into) {
                    *o = __builtin_nan("");
                }
            }
    }
    return launch(true);
}
// norms_plan.hpp's value and walk (norms_walk, the function the kernel calls) under extremes_plan.hpp's rule; a unit is one run of a probe
hipError_t launch_history_norms(const NormsArgs& a, uint32_t n_probes, double* out, void* scratch, uint32_t segments, bool merge_into, uint64_t n, uint32_t period,
                                uint64_t first_tick, uint64_t n_samples, uint64_t every, uint64_t ring, size_t elem, hipStream_t s) {
    if (deferring())
        return defer_scan(s, "history_norms", {out, scratch}, n_probes, kNormsMaxProbes, [&](uint32_t c, auto& dev) { probe_rings(a.p[c], dev); }, [=] {
            return launch_history_norms(a, n_probes, out, scratch, segments, merge_into, n, period, first_tick, n_samples, every, ring, elem, s);
        });
    if (!norms_launch_ok(a, n_probes, n, period, first_tick, n_samples, every, segments) || ring == 0) return launch(false);
    if (n == 0) return launch(true);
    const uint64_t runs = n / period, units = runs * n_probes;
    if (segments > 1 && !need(live(scratch, scan_scratch_bytes(segments, units, kNormsFields)), "norms scratch records")) return launch(false);
    if (!need(live(out, units * kNormsPlanes * sizeof(double)), "norms staging")) return launch(false);
    for (uint32_t k = 0; k < n_probes; k++) {
        const NormsProbe& p = a.p[k];
        if (!need(probe_live(p, ring, n, elem), "ring of a probe")) return launch(false);
        with_elem(elem, [&](auto e) {
            using E = decltype(e);
            scan_stages(planes_acc<double>(runs, [&](uint64_t run) { return out + norms_out_index(k, runs, run); }), runs, runs, segments, merge_into, n_samples,
                        [&](uint64_t run, uint64_t lo, uint64_t hi, const ExtremesRecord& start) { return norms_walk<E>(start, p, run, n, period, lo, hi, first_tick, every, ring); },
                        [&](uint32_t seg, uint64_t run) { return static_cast<uint64_t*>(scratch) + norms_scratch_index(seg, n_probes, k, runs, run); });
        });
    }
    return launch(true);
}
// norm_events_plan.hpp's walk (norm_events_walk, the function the kernel calls) under events_plan.hpp's rule; a unit is one run of a trigger
hipError_t launch_history_norm_events(const NormEventsArgs& a, uint32_t n_triggers, void* rec, double* out, void* scratch, uint32_t segments, bool merge_into, uint64_t n,
                                      uint32_t period, uint64_t first_tick, uint64_t n_samples, uint64_t every, uint64_t ring, size_t elem, hipStream_t s) {
    if (deferring())
        return defer_scan(s, "history_norm_events", {rec, out, scratch}, n_triggers, kNormEventsMaxTriggers, [&](uint32_t c, auto& dev) { probe_rings(a.t[c].probe, dev); }, [=] {
            return launch_history_norm_events(a, n_triggers, rec, out, scratch, segments, merge_into, n, period, first_tick, n_samples, every, ring, elem, s);
        });
    if (!norm_events_launch_ok(a, n_triggers, n, period, first_tick, n_samples, every, segments) || ring == 0) return launch(false);
    if (n == 0) return launch(true);
    const uint64_t runs = n / period, units = runs * n_triggers;
    if (segments > 1 && !need(live(scratch, scan_scratch_bytes(segments, units, kNormEventsFields)), "norm events scratch records")) return launch(false);
    if (!need(live(rec, events_record_bytes(units)) && live(out, units * kNormEventsPlanes * sizeof(double)), "norm events records or staging")) return launch(false);
    for (uint32_t k = 0; k < n_triggers; k++) {
        const NormEventsTrigger& t = a.t[k];
        if (!need(probe_live(t.probe, ring, n, elem), "ring of a trigger's probe")) return launch(false);
        with_elem(elem, [&](auto e) {
            using E = decltype(e);
            scan_stages(records_acc<double>(runs, t.mode, [&](uint64_t run) { return static_cast<uint64_t*>(rec) + norm_events_record_index(k, runs, run); },
                                            [&](uint64_t run) { return out + norm_events_out_index(k, runs, run); }),
                        runs, runs, segments, merge_into, n_samples,
                        [&](uint64_t run, uint64_t lo, uint64_t hi, const EventsRecord& start) { return norm_events_walk<E>(start, t, run, n, period, lo, hi, first_tick, every, ring); },
                        [&](uint32_t seg, uint64_t run) { return static_cast<uint64_t*>(scratch) + norm_events_scratch_index(seg, n_triggers, k, runs, run); });
        });
    }
    return launch(true);
}
// dwell_plan.hpp's value, walk (dwell_walk, the function the kernel calls) and rule; a unit is one run of a condition
hipError_t launch_history_dwell(const DwellArgs& a, uint32_t n_conditions, double* out, void* scratch, uint32_t segments, bool merge_into, uint64_t n, uint32_t period,
                                uint64_t first_tick, uint64_t n_samples, uint64_t every, uint64_t ring, size_t elem, hipStream_t s) {
    if (deferring())
        return defer_scan(s, "history_dwell", {out, scratch}, n_conditions, kDwellMaxConditions, [&](uint32_t c, auto& dev) { probe_rings(a.c[c].probe, dev); }, [=] {
            return launch_history_dwell(a, n_conditions, out, scratch, segments, merge_into, n, period, first_tick, n_samples, every, ring, elem, s);
        });
    if (!dwell_launch_ok(a, n_conditions, n, period, first_tick, n_samples, every, segments) || ring == 0) return launch(false);
    if (n == 0) return launch(true);
    const uint64_t runs = n / period, units = runs * n_conditions;
    if (segments > 1 && !need(live(scratch, scan_scratch_bytes(segments, units, kDwellFields)), "dwell scratch records")) return launch(false);
    if (!need(live(out, units * kDwellPlanes * sizeof(double)), "dwell staging")) return launch(false);
    for (uint32_t k = 0; k < n_conditions; k++) {
        const DwellCondition& c = a.c[k];
        if (!need(probe_live(c.probe, ring, n, elem), "ring of a condition's probe")) return launch(false);
        with_elem(elem, [&](auto e) {
            using E = decltype(e);
            scan_stages(dwell_planes_acc(runs, [&](uint64_t run) { return out + dwell_out_index(k, runs, run); }), runs, runs, segments, merge_into, n_samples,
                        [&](uint64_t run, uint64_t lo, uint64_t hi, const DwellRecord& start) { return dwell_walk<E>(start, c, run, n, period, lo, hi, first_tick, every, ring); },
                        [&](uint32_t seg, uint64_t run) { return static_cast<uint64_t*>(scratch) + dwell_scratch_index(seg, n_conditions, k, runs, run); });
        });
    }
    return launch(true);
}
hipError_t launch_nonfinite(const void* pos, const void* vel, uint32_t n, size_t elem, uint8_t* flags, unsigned long long* count, hipStream_t s) {
    if (deferring()) return defer(s, "count_nonfinite", {pos, vel, flags, count}, [=] { return launch_nonfinite(pos, vel, n, elem, flags, count, s); });
    return launch(need(live(pos, n * 7 * elem) && live(vel, n * 6 * elem) && live(count, 8) && (!flags || live(flags, n)), "count_nonfinite buffers"));
}

// no HSA queue here: the host layer stays on its hipGraph / eager path
namespace aql {
Device* acquire(int, std::string* why) { return *why = "no HSA queue in the host-only build", nullptr; }
void release(Device*) {}
bool kernel_code(Device*, const void*, uint32_t, KernelCode*, std::string* why) { return *why = "no HSA queue", false; }
bool run_chain(Device*, const Run*, size_t, double, double*, std::string* why) { return *why = "no HSA queue", false; }
}  // namespace aql

}  // namespace sixdof
