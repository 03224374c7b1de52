// sixdof_capi.cpp — host side of the C ABI declared in include/sixdof_hip.h.
//
// Mirrors the reference's backend object (CraneliftExec / JaxExec,
// libs/nox-py/src/cranelift_exec.rs:13-195, jax_exec.rs:118-185): it owns the slot tables and
// the device-resident copies of the ECS columns, runs batches of ticks, and copies columns
// back on request.  Differences that are the point of this backend: columns stay resident in
// HBM between batches (the JAX backend re-uploads every input and downloads every output per
// batch), and a batch is one or a few kernel launches instead of a per-tick host loop.
//
// No CPU fallback exists: every entry point that needs the GPU fails with SIXDOF_ERR_NO_DEVICE /
// SIXDOF_ERR_BACKEND when HIP is unavailable.
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/sixdof_hip.h"
#include "../../include/sixdof_apollo.h"
#include "kernels.hpp"
#include "abi_guard.hpp"
#include "device_mem.hpp"
#include "aql_chain.hpp"
#include "covariance_plan.hpp"
#include "envelope_plan.hpp"
#include "events_plan.hpp"
#include "norms_plan.hpp"
#include "dwell_plan.hpp"
#include "norm_events_plan.hpp"
#include "extremes_plan.hpp"
#include "quantile_plan.hpp"
#include "history_plan.hpp"
#include "step_plan.hpp"

using namespace sixdof;

namespace {

struct Column {
    uint64_t id = 0;
    int prim = SIXDOF_PRIM_F64;
    uint64_t width = 1;  // elements per row
    uint64_t n_rows = 0;
    size_t elem = 8;
    size_t bytes = 0;
    std::vector<uint64_t> ids;
    void* host = nullptr;  // borrowed
    DeviceBuffer dev;      // the full column, reference byte layout
    // join state: rows of this column that belong to the joined entity set, in joined order.  `live` is what
    // the kernels read and write: == dev when the column IS the joined set, else an owned compact [m,w] copy.
    std::vector<uint32_t> rows;
    DeviceBuffer d_rows, compact;
    void* live = nullptr;
    bool joined = false;   // join resolved for the current binding
    DeviceBuffer snap;     // device snapshot the async telemetry copy reads (sixdof_download_async)
    PinnedRange host_pinned;    // the host buffer, once page-locked by us

    void drop_join() {
        d_rows.reset(), compact.reset();
        rows.clear();
        live = nullptr;
        joined = false;
    }
};

thread_local std::string g_create_error;

// What the fold kernels of a generated program with device fold tables take next to StepParams (elodin_amd/codegen.py emits the
// same struct into the object, which reports its size: sixdof_custom_fold_info).  Sources [0, n_lane) are folded by one lane each,
// [n_lane, n_src) by one wave each.
struct FoldTable {
    const uint32_t* src_rows;
    const uint32_t* row_start;
    const uint32_t* dst;
    uint32_t n_src;
    uint32_t n_lane;
};
constexpr uint32_t kFoldWaveDegree = 64;   // out-degree from which a regroupable fold gives a source a whole wave

// One fold stage of the installed generated program, as the object describes it, and the table it currently reads.
struct FoldSlot {
    bool needs_table = false;   // false: the complete graph over a world's rows (arithmetic, no table)
    bool wave_ok = false;       // a plain sum that asked for waves: long sources go behind n_lane
    uint32_t count = 1, stride = 0;   // replicas the object was generated for (1, 0: none)
    bool set = false;
    DeviceBuffer d_blob;              // [src_rows | row_start | dst]
    FoldTable table{};
};
using SetFoldTableFn = int (*)(unsigned, const FoldTable*);

double now_ms() {
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

uint64_t cid(const char* s) { return sixdof_component_id(s); }

constexpr uint32_t kAqlSlots = 8;   // argument blocks of AQL chains per handle (Replay::aql_args)
constexpr uint32_t kAqlSpare0 = 3;  // slots 0 .. 2: the K-tick launches (plain, accel check, state-only); the rest are spares

// What the step kernel's batches replay: captured hipGraphs, and the queue and argument blocks of AQL chains (aql_chain.hpp).
// Both are built from `key` and dropped together.
struct Replay {
    // Everything a replayed launch bakes in: the batch's StepParams (column pointers, n, both time steps, effector ops, cache
    // policy) with n_ticks = K and tick0 = hist_slot0 = 0 (read only off the graph-eligible paths); state_only stays 0 like
    // accel_in_check: both are set per launch.  Integrator and dtype are fixed per handle.
    StepParams key{};
    std::map<uint32_t, hipGraphExec_t> graphs;   // replay graphs by graph_key(chain length, variant)
    bool state_only_off = false;            // SIXDOF_STATE_ONLY=0 when the handle was created: every launch stores all four columns
    bool aql_off = false;                   // SIXDOF_AQL=0 when the handle was created: keep the hipGraph path
    aql::Device* aql_dev = nullptr;
    std::string aql_why;                    // why AQL setup failed (the hipGraph path then stays); not retried
    std::string aql_fault;                  // a chain failed on the queue: every later step fails with this
    DeviceBuffer aql_args;                  // device arena of argument blocks (kAqlSlots)
    std::map<uint64_t, aql::Run> aql_runs;  // by (state_only, accel_in_check, n_ticks): kernel, argument block, grid
    uint64_t aql_slot_key[kAqlSlots] = {};  // the run whose block each spare slot (kAqlSpare0 ..) holds, 0: none
    uint32_t aql_next_spare = kAqlSpare0;   // the spare slot the next new run takes

    void drop() {
        for (auto& kv : graphs) hipGraphExecDestroy(kv.second);
        graphs.clear();
        aql_runs.clear();
        std::fill(std::begin(aql_slot_key), std::end(aql_slot_key), 0);
        aql_next_spare = kAqlSpare0;
    }
    // `P`: a batch's parameters (n_ticks = K).  Whatever was built from other parameters is dropped.
    void rekey(StepParams P) {
        P.tick0 = P.hist_slot0 = 0;   // fill_step_params memsets the struct: the padding compares equal too
        if (std::memcmp(&P, &key, sizeof(P)) != 0) drop(), key = P;
    }
    void release() {
        drop();
        if (!aql_fault.empty()) (void)aql_args.release();   // leaked: after a failed chain a dispatch may still read it
        aql_args.reset();
        aql::release(aql_dev);
    }
};

// What sixdof_set_edges replaces as one: built in a local, swapped in after the last call that can fail.
struct Edges {
    std::vector<uint32_t> src, dst;              // resolved rows, spawn order
    DeviceBuffer d_csr_start, d_csr_dst;         // CSR by source, spawn order kept inside a source
    // hub sources of the edge list (out-degree >= kHubDegree): one device block [hub_rows | hub_chunk_start | chunk_e0 | chunk_row]
    DeviceBuffer d_hub, d_chunk_partial;
    uint32_t n_hubs = 0, n_hub_chunks = 0;
};

// The telemetry ring.  reset() is the state without one: a ring is complete (every buffer allocated) or absent.
struct History {
    uint32_t ring = 0;
    uint64_t first_tick = 0;          // first tick (1-based count) recorded since the ring was enabled
    DeviceBuffer body[4];             // pos, vel, accel, force
    std::vector<DeviceBuffer> model;  // one ring per component column of a generated program (same order as custom_model; empty: not recorded)
    // sixdof_history_envelope: device staging of one read's output and the stage-1 partial records, grown lazily, freed with the ring
    DeviceBuffer env_stage, env_partial;
    // sixdof_history_quantiles: its staging, and the histograms and slot states of one launch; the same rules
    DeviceBuffer quant_stage, quant_scratch;
    // sixdof_history_covariance: its staging and the stage-1 partial records of one launch; the same rules
    DeviceBuffer cov_stage, cov_partial;
    // A scan over time (time_scan_read: sixdof_history_extremes, sixdof_history_events, sixdof_history_norms, sixdof_history_norm_events, sixdof_history_dwell): its staging, which is also the accumulator
    // a *_CONTINUE call merges into, the segment records of one launch and — the two event readers only — the records its rule continues
    // from; the same rules.  `acc` says what the accumulator holds, if anything.
    struct ScanState {
        bool valid = false;                  // the previous call succeeded and nothing has replaced what it read since
        std::vector<uint64_t> signature;     // what was asked for, in plain words: the same request gives the same words
        std::vector<const void*> rings;      // ring base and width of everything read, as they were: a replaced program changes them
        std::vector<size_t> widths;
        uint64_t n = 0;
        uint64_t last_tick = 0;              // the last tick accumulated
    };
    struct TimeScan {
        DeviceBuffer stage, scratch, rec;
        ScanState acc;
    } extremes, events, norms, norm_events, dwell;
    void reset() { *this = History{}; }
};

// The telemetry D2H lane that overlaps the compute stream: its stream and two events exist together or not at all.
// Every asynchronous read-back (sixdof_download_async, sixdof_history_stream, StagedRead::deliver) is
//     [hold]  what its copies read is made ready on the compute stream  begin  copy ...  end
// and a failure anywhere leaves `pending` as it was: nothing new to wait for, the next call starts afresh.
struct CopyLane {
    Stream stream;
    Event ev_snap, ev_copied;
    bool pending = false;
    uint64_t stream_lo = 1, stream_hi = 0;   // ticks of the history runs whose copies may still be in flight (hi < lo: none)
    std::vector<PinnedRange> pinned_user;    // caller's buffers page-locked by sixdof_history_stream / sixdof_watch_read, until sixdof_sync
    // Before `compute` overwrites a buffer the copies of an earlier read take their data from (snapshots, a staging buffer):
    // those copies must have drained it.  A device-side wait; the host goes on.
    hipError_t hold(hipStream_t compute) { return pending ? hipStreamWaitEvent(compute, ev_copied.get(), 0) : hipSuccess; }
    // The copies that follow start once everything enqueued on `compute` so far has completed.
    hipError_t begin(hipStream_t compute) {
        hipError_t e = ensure();
        if (e == hipSuccess) e = hipEventRecord(ev_snap.get(), compute);
        if (e == hipSuccess) e = hipStreamWaitEvent(stream.get(), ev_snap.get(), 0);
        return e;
    }
    // One D2H on the copy stream; [dst, dst + pin_bytes) is page-locked first (0: the caller's business).
    hipError_t copy(void* dst, const void* src, size_t bytes, size_t pin_bytes) {
        if (pin_bytes)
            if (hipError_t e = pin(dst, pin_bytes); e != hipSuccess) return e;
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream.get());
    }
    // ev_copied is re-recorded behind whatever the copy stream already carried: one sixdof_download_wait covers every read
    // enqueued before it, of whichever kind.
    hipError_t end() {
        hipError_t e = hipEventRecord(ev_copied.get(), stream.get());
        if (e == hipSuccess) pending = true;
        return e;
    }
    hipError_t ensure() {
        if (stream) return hipSuccess;
        Stream s;
        Event a, b;
        hipError_t e = hipStreamCreateWithFlags(s.out(), hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(a.out(), hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(b.out(), hipEventDisableTiming);
        if (e != hipSuccess) return e;
        stream = std::move(s), ev_snap = std::move(a), ev_copied = std::move(b);
        return hipSuccess;
    }
    // Before [p, p + bytes) becomes the host side of a copy: a lock of ours either covers all of it (*covered) or does not touch
    // it.  A lock that covers only a part — an earlier, shorter read into the same buffer — is dropped, once the copies that may
    // still run under it have landed: what the runtime makes of a partly locked range is nowhere specified.
    hipError_t settle(const void* p, size_t bytes, bool* covered = nullptr) {
        bool partly = false, whole = false;
        for (const PinnedRange& r : pinned_user) {
            whole = whole || r.contains(p, bytes);   // locks are disjoint: then no other touches it
            partly = partly || r.intersects(p, bytes);
        }
        if (covered) *covered = whole;
        if (whole || !partly) return hipSuccess;
        if (stream)
            if (hipError_t e = hipStreamSynchronize(stream.get()); e != hipSuccess) return e;
        pinned_user.erase(std::remove_if(pinned_user.begin(), pinned_user.end(), [&](const PinnedRange& r) { return r.intersects(p, bytes); }), pinned_user.end());
        return hipSuccess;
    }
    // page-lock once, the whole range; if it cannot be locked the copy still works, staged
    hipError_t pin(void* p, size_t bytes) {
        bool covered = false;
        if (hipError_t e = settle(p, bytes, &covered); e != hipSuccess || covered) return e;
        PinnedRange r;
        if (r.lock(p, bytes)) pinned_user.push_back(std::move(r));
        return hipSuccess;
    }
};

// The Body archetype (six_dof.rs:152-159).  `ring`: index of the column's history ring (History::body), -1: not recorded.
struct BodyCol {
    const char* name;
    uint64_t width;
    uint32_t bit;   // SIXDOF_COL_*
    int ring;
    uint64_t id;
};

// entity id -> row
using RowMap = std::unordered_map<uint64_t, uint32_t>;
RowMap row_map(const std::vector<uint64_t>& ids) {
    RowMap m;
    m.reserve(ids.size() * 2);
    for (size_t r = 0; r < ids.size(); r++) m.emplace(ids[r], static_cast<uint32_t>(r));
    return m;
}
// rows[i] = row of ids[i]; returns n, or the index of the first id the map does not hold
size_t resolve_rows(const RowMap& m, const uint64_t* ids, size_t n, std::vector<uint32_t>* rows) {
    rows->resize(n);
    for (size_t i = 0; i < n; i++) {
        auto it = m.find(ids[i]);
        if (it == m.end()) return i;
        (*rows)[i] = it->second;
    }
    return n;
}

}  // namespace

// Members are destroyed in reverse order: streams and events last, after everything that was used on them.
struct sixdof_handle {
    sixdof_desc desc{};
    int device = 0;
    Stream stream;
    Event ev0, ev1;
    Event evp0, evp1;  // the pair the PREVIOUS asynchronous step recorded (two pairs alternate)
    bool prev_pending = false;
    CopyLane copy;
    bool step_pending = false;                  // SIXDOF_FLAG_ASYNC_STEP: ev1 of the last step not yet read
    std::vector<Event> launch_events;  // SIXDOF_FLAG_TIME_EACH_LAUNCH: 2 per launch
    std::map<uint64_t, Column> cols;  // ascending ComponentId = reference BTreeMap order
    std::vector<sixdof_effector_op> ops;
    Edges edges;
    DeviceBuffer d_scratch;            // pair-path scratch
    std::vector<uint64_t> joined_ids;  // intersection of the Body columns' entity ids (query.rs:136-208)
    bool identity_join = true;         // every Body column already is the joined set (query.rs:673,702 fast path)
    uint64_t tick = 0;
    bool bound = false;
    bool resident = false;             // columns uploaded at least once since the last bind
    sixdof_timings last{};   // most recent upload / step / download
    // run-time generated effector pipe
    DlHandle custom_dl;
    CustomLaunchFn custom_launch = nullptr;
    DlHandle pair_dl;                      // generated edge_fold function (sixdof_set_custom_pair)
    CustomPairLaunchFn pair_launch = nullptr;
    std::vector<uint64_t> custom_aux;      // read-only [n,1..3] columns of a generated effector pipe
    std::vector<uint64_t> custom_model;    // read/write [n,1..16] component columns of a generated program
    bool custom_tick_free = false;          // the generated program never looks at the absolute tick (layout bit 17): replayable
    int pair_only_small = -1;               // what the installed pair object was generated for (-1: both launch shapes)
    unsigned custom_rows_multiple = 1;      // rows a world of the generated program occupies (lane mode): the joined row count must be a multiple
    // fold stages of a generated program that reads its edges from device memory (empty: none, or a baked object)
    SetFoldTableFn custom_set_fold_table = nullptr;
    std::vector<FoldSlot> custom_folds;
    History hist;
    std::vector<unsigned> custom_model_width;   // what the generated code expects per column (0 = unknown), bit 31 = window
    // watch list (sixdof_set_watch): the components and joined rows whose series sixdof_watch_read gathers out of the ring.
    // Only ids and rows are kept: ring base pointers and widths are looked up per read, so the ring may come, go or be
    // re-sized in between.
    std::vector<uint64_t> watch_ids;
    DeviceBuffer d_watch_rows;
    size_t watch_m = 0;
    DeviceBuffer d_watch_stage;           // device staging of one read, grown lazily
    // rollout model (0 = none, 1 = Apollo lander)
    int model = 0;
    std::vector<double> ap_time, ap_alt, ap_rate, ap_pitch, ap_hspeed, ap_downrange;
    bool accel_is_host_data = false;   // set by an upload: the next RK4 launch reads world_accel once (see sixdof_step)
    uint32_t ap_ticks_per_telemetry = 3;
    uint32_t ap_guidance_period = 5;
    uint64_t ap_max_ticks = 0;
    DeviceBuffer d_tick_refs;
    Replay replay;
    std::string path;                       // sixdof_step_path's answer
    mutable std::string err;

    BodyCol body[5] = {{"world_pos", 7, SIXDOF_COL_WORLD_POS, 0, 0},     {"world_vel", 6, SIXDOF_COL_WORLD_VEL, 1, 0},
                       {"world_accel", 6, SIXDOF_COL_WORLD_ACCEL, 2, 0}, {"force", 6, SIXDOF_COL_FORCE, 3, 0},
                       {"inertia", 7, SIXDOF_COL_INERTIA, -1, 0}};
    uint64_t id_pos, id_vel, id_accel, id_force, id_inertia, id_tick, id_dt;

    int fail(int code, const std::string& msg) const {
        err = msg;
        return code;
    }
    int hip_fail(hipError_t e, const char* what) const {
        err = std::string(what) + ": " + hipGetErrorString(e);
        return SIXDOF_ERR_BACKEND;
    }
    Column* col(uint64_t id) {
        auto it = cols.find(id);
        return it == cols.end() ? nullptr : &it->second;
    }
    const Column* col(uint64_t id) const {
        auto it = cols.find(id);
        return it == cols.end() ? nullptr : &it->second;
    }
    size_t elem_size() const { return desc.dtype == SIXDOF_F32 ? 4 : 8; }
    int state_prim() const { return desc.dtype == SIXDOF_F32 ? SIXDOF_PRIM_F32 : SIXDOF_PRIM_F64; }
    // the caller has drained the compute stream (a gather may still read the table)
    void drop_watch() {
        d_watch_rows.reset();
        watch_ids.clear();
        watch_m = 0;
    }
    bool has_pair_op() const {
        for (auto& o : ops)
            if (SIXDOF_EFF_IS_PAIR(o.kind)) return true;
        return false;
    }
};

// where the exception barrier (abi_guard.hpp) leaves its message: the handle's error, or the creation error without a handle
std::string* err_of(const sixdof_handle* h) { return h ? &const_cast<sixdof_handle*>(h)->err : &g_create_error; }

#define HIP_TRY(h, call)                                      \
    do {                                                      \
        hipError_t e_ = (call);                               \
        if (e_ != hipSuccess) return (h)->hip_fail(e_, #call); \
    } while (0)

// Map the joined entity set onto one column: `rows[j]` = row of joined entity j in this column.  Identity ->
// kernels work on the column itself; otherwise on a compact [m,w] copy (gathered on upload, scattered on download).
static int resolve_join(sixdof_handle* h, Column* c) {
    if (c->joined) return SIXDOF_OK;
    const size_t m = h->joined_ids.size();
    if (c->ids == h->joined_ids) {
        c->live = c->dev.get();
        c->joined = true;
        return SIXDOF_OK;
    }
    std::vector<uint32_t> rows;
    if (resolve_rows(row_map(c->ids), h->joined_ids.data(), m, &rows) != m)
        return h->fail(SIXDOF_ERR_ENTITY_MISMATCH, "join: a column does not cover the joined Body entity set");
    DeviceBuffer d_rows, compact;
    if (m) {
        HIP_TRY(h, d_rows.alloc(m * sizeof(uint32_t)));
        HIP_TRY(h, hipMemcpy(d_rows.get(), rows.data(), m * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_TRY(h, compact.alloc(m * c->width * c->elem));
    }
    c->rows.swap(rows);
    c->d_rows = std::move(d_rows), c->compact = std::move(compact);
    c->live = c->compact.get();
    c->joined = true;
    return SIXDOF_OK;
}

// the joined rows of a column whose full copy changed (an upload): full column -> compact copy, on the compute stream
static int gather_joined(sixdof_handle* h, Column* c) {
    if (!c->joined || !c->compact) return SIXDOF_OK;
    hipError_t e = launch_gather_rows(c->compact.get(), c->dev.get(), c->d_rows.get<uint32_t>(), static_cast<uint32_t>(h->joined_ids.size()),
                                      static_cast<uint32_t>(c->width), c->elem, h->stream.get());
    return e == hipSuccess ? SIXDOF_OK : h->hip_fail(e, "gather_rows");
}

// first use of a column after binding: join it onto the Body set and bring its rows over
static int ensure_joined(sixdof_handle* h, Column* c) {
    if (c->joined) return SIXDOF_OK;
    int rc = resolve_join(h, c);
    return rc != SIXDOF_OK ? rc : gather_joined(h, c);
}

// H2D of one column, then the gather of its joined rows: enqueued, the caller waits for the compute stream
static int upload_one(sixdof_handle* h, Column* c) {
    if (c->bytes) HIP_TRY(h, hipMemcpyAsync(c->dev.get(), c->host, c->bytes, hipMemcpyHostToDevice, h->stream.get()));
    return gather_joined(h, c);
}

extern "C" {

uint32_t sixdof_abi_version(void) { return SIXDOF_ABI_VERSION; }

// sixdof_component_id / sixdof_quantize_time_step: pure host code, in world.cpp (so the host layer links without HIP: `make asan`)

int sixdof_device_count(void) try {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
} SIXDOF_ABI_CATCH(&g_create_error)

const char* sixdof_last_error(const sixdof_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

void sixdof_destroy(sixdof_handle* h);

int sixdof_create(const sixdof_desc* d, sixdof_handle** out) try {
    if (!d || !out) {
        g_create_error = "sixdof_create: null argument";
        return SIXDOF_ERR_INVALID_ARGUMENT;
    }
    *out = nullptr;
    if (d->struct_size != sizeof(sixdof_desc)) {
        g_create_error = "sixdof_create: struct_size mismatch (ABI version skew)";
        return SIXDOF_ERR_INVALID_ARGUMENT;
    }
    if (d->integrator != SIXDOF_INTEGRATOR_RK4 && d->integrator != SIXDOF_INTEGRATOR_SEMI_IMPLICIT &&
        d->integrator != SIXDOF_INTEGRATOR_NONE) {
        g_create_error = "sixdof_create: unknown integrator";
        return SIXDOF_ERR_INVALID_ARGUMENT;
    }
    if (d->dtype != SIXDOF_F64 && d->dtype != SIXDOF_F32) {
        g_create_error = "sixdof_create: unknown dtype";
        return SIXDOF_ERR_INVALID_ARGUMENT;
    }
    if (d->n_entities > 0xFFFFFFF0ull) {
        g_create_error = "sixdof_create: n_entities exceeds u32 row index range";
        return SIXDOF_ERR_INVALID_ARGUMENT;
    }
    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev == 0) {
        g_create_error = std::string("sixdof_create: no HIP device (") + hipGetErrorString(e) +
                         "); this backend has no CPU fallback";
        return SIXDOF_ERR_NO_DEVICE;
    }
    if (d->device_ordinal < 0 || d->device_ordinal >= n_dev) {
        g_create_error = "sixdof_create: device_ordinal out of range";
        return SIXDOF_ERR_INVALID_ARGUMENT;
    }
    auto* h = new sixdof_handle();
    h->desc = *d;
    if (h->desc.ticks_per_launch == 0) h->desc.ticks_per_launch = 1;
    const char* aql_env = std::getenv("SIXDOF_AQL");   // "0": hipGraph replay instead of AQL chains (A/B runs)
    h->replay.aql_off = aql_env && aql_env[0] == '0';
    const char* so_env = std::getenv("SIXDOF_STATE_ONLY");   // "0": every launch stores world_accel and force (A/B runs, tests)
    h->replay.state_only_off = so_env && so_env[0] == '0';
    h->device = d->device_ordinal;
    for (BodyCol& b : h->body) b.id = cid(b.name);
    h->id_pos = h->body[0].id, h->id_vel = h->body[1].id, h->id_accel = h->body[2].id, h->id_force = h->body[3].id;
    h->id_inertia = h->body[4].id;
    h->id_tick = cid("tick");
    h->id_dt = cid("simulation_time_step");
    if ((e = hipSetDevice(h->device)) != hipSuccess || (e = hipStreamCreate(h->stream.out())) != hipSuccess ||
        (e = hipEventCreate(h->ev0.out())) != hipSuccess || (e = hipEventCreate(h->ev1.out())) != hipSuccess ||
        (e = hipEventCreate(h->evp0.out())) != hipSuccess || (e = hipEventCreate(h->evp1.out())) != hipSuccess) {
        g_create_error = std::string("sixdof_create: ") + hipGetErrorString(e);
        sixdof_destroy(h);   // releases whatever part was created
        return SIXDOF_ERR_BACKEND;
    }
    *out = h;
    return SIXDOF_OK;
} SIXDOF_ABI_CATCH(&g_create_error)

void sixdof_destroy(sixdof_handle* h) try {
    if (!h) return;
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream.get());
    if (h->copy.stream) hipStreamSynchronize(h->copy.stream.get());
    h->replay.release();
    delete h;   // the owners release the rest (device_mem.hpp), in reverse order of declaration
} SIXDOF_ABI_CATCH_VALUE(err_of(h), )

int sixdof_bind_columns(sixdof_handle* h, const sixdof_column* cols, size_t n_cols) try {
    if (!h || (!cols && n_cols)) return SIXDOF_ERR_INVALID_ARGUMENT;
    h->bound = h->resident = false;   // until the end of this call: a failed bind leaves the handle unbound
    h->hist.extremes.acc.valid = h->hist.events.acc.valid = h->hist.norms.acc.valid = h->hist.norm_events.acc.valid = h->hist.dwell.acc.valid = false;   // the rows a scan's accumulator covers may be other rows from here on
    HIP_TRY(h, hipSetDevice(h->device));
    h->replay.drop();
    if (h->d_watch_rows) {      // a watch holds rows of the join this call replaces
        HIP_TRY(h, hipStreamSynchronize(h->stream.get()));
        h->drop_watch();
    }
    for (size_t i = 0; i < n_cols; i++) {
        const sixdof_column& c = cols[i];
        if (c.ndim > 1) return h->fail(SIXDOF_ERR_UNSUPPORTED, "bind_columns: only scalar / 1-D components");
        if (!c.host_ptr && c.n_rows) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, "bind_columns: null host_ptr");
        Column col;
        col.id = c.component_id;
        col.prim = c.prim_type;
        col.width = c.ndim == 0 ? 1 : c.dims[0];
        col.n_rows = c.n_rows;
        col.elem = c.prim_type == SIXDOF_PRIM_F32 ? 4 : 8;
        col.bytes = static_cast<size_t>(col.width * col.n_rows) * col.elem;
        col.host = c.host_ptr;
        if (c.entity_ids) col.ids.assign(c.entity_ids, c.entity_ids + c.n_rows);
        if (Column* old = h->col(c.component_id)) {
            if (old->bytes == col.bytes) col.dev = std::move(old->dev);
            // the copy lane may still read the previous binding's snapshot and write its (page-locked) host buffer
            if (h->copy.stream) HIP_TRY(h, hipStreamSynchronize(h->copy.stream.get()));
        }
        if (!col.dev && col.bytes) HIP_TRY(h, col.dev.alloc(col.bytes));
        // the previous binding's join tables, snapshot (sized per binding) and page lock (of its host buffer) go with its entry
        h->cols[c.component_id] = std::move(col);
    }
    // six_dof's queries run over the INTERSECTION of the Body columns' entity ids in ascending id order
    // (query.rs:136-208); rows outside it are never touched.
    const Column* first = nullptr;
    bool identical = true;
    for (auto& b : h->body) {
        const Column* c = h->col(b.id);
        if (!c) return h->fail(SIXDOF_ERR_COMPONENT_NOT_FOUND, std::string("bind_columns: missing Body column ") + b.name);
        if (c->prim != h->state_prim())
            return h->fail(SIXDOF_ERR_VALUE_SIZE_MISMATCH, std::string("bind_columns: dtype mismatch on ") + b.name);
        if (c->width != b.width)
            return h->fail(SIXDOF_ERR_VALUE_SIZE_MISMATCH, std::string("bind_columns: shape mismatch on ") + b.name);
        if (c->ids.size() != c->n_rows)
            return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, std::string("bind_columns: entity_ids missing on ") + b.name);
        if (!first) first = c;
        else if (c->ids != first->ids) identical = false;
    }
    if (identical) {
        h->joined_ids = first->ids;   // fast path: column order as is (query.rs:673,702)
    } else {
        std::vector<uint64_t> acc(first->ids);
        std::sort(acc.begin(), acc.end());
        for (auto& b : h->body) {
            std::vector<uint64_t> ids(h->col(b.id)->ids), out;
            std::sort(ids.begin(), ids.end());
            std::set_intersection(acc.begin(), acc.end(), ids.begin(), ids.end(), std::back_inserter(out));
            acc.swap(out);
        }
        h->joined_ids.swap(acc);      // ascending entity id
    }
    h->identity_join = identical;
    if (h->desc.n_entities == 0) h->desc.n_entities = h->joined_ids.size();
    // a generated program installed BEFORE the join was sized (n_entities == 0 then: its whole-worlds check passed on nothing)
    if (h->custom_rows_multiple > 1 && h->desc.n_entities % h->custom_rows_multiple != 0)
        return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, "bind_columns: the installed program lays a world out as " + std::to_string(h->custom_rows_multiple) +
                       " consecutive rows; the joined " + std::to_string(h->desc.n_entities) + " rows are not a whole number of worlds");
    if (h->joined_ids.size() != h->desc.n_entities)
        return h->fail(SIXDOF_ERR_VALUE_SIZE_MISMATCH, "bind_columns: n_entities does not match the joined Body entity set");
    for (auto& kv : h->cols) kv.second.drop_join();
    for (auto& b : h->body) {
        int rc = resolve_join(h, h->col(b.id));
        if (rc != SIXDOF_OK) return rc;
    }
    h->bound = true;
    return SIXDOF_OK;
} SIXDOF_ABI_CATCH(err_of(h))

int sixdof_bind_world(sixdof_handle* h, sixdof_world* w) try {
    if (!h || !w) return SIXDOF_ERR_INVALID_ARGUMENT;
    std::vector<uint64_t> ids(sixdof_world_components(w, nullptr, 0));
    sixdof_world_components(w, ids.data(), ids.size());
    std::vector<sixdof_column> cols;
    for (uint64_t id : ids) {
        sixdof_column c{};
        if (sixdof_world_column(w, id, &c) != SIXDOF_OK) continue;
        if (id == h->id_tick || id == h->id_dt) continue;   // globals travel in the descriptor / handle
        if (c.prim_type != h->state_prim() || c.ndim > 1) continue;
        cols.push_back(c);
    }
    h->desc.simulation_time_step = sixdof_world_time_step(w);
    h->tick = sixdof_world_tick(w);
    return sixdof_bind_columns(h, cols.data(), cols.size());
} SIXDOF_ABI_CATCH(err_of(h))

int sixdof_set_effectors(sixdof_handle* h, const sixdof_effector_op* ops, size_t n_ops) try {
    if (!h || (!ops && n_ops)) return SIXDOF_ERR_INVALID_ARGUMENT;
    size_t n_entity_ops = 0, n_pair = 0;
    for (size_t i = 0; i < n_ops; i++) {
        const int k = ops[i].kind;
        if (k < SIXDOF_EFF_CONST_WRENCH || k > SIXDOF_EFF_WORLD_FORCE || k == SIXDOF_EFF_EDGE_CUSTOM)
            return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, "set_effectors: unknown effector kind");
        if (SIXDOF_EFF_IS_PAIR(k)) {
            n_pair++;
            if (i + 1 != n_ops)
                return h->fail(SIXDOF_ERR_UNSUPPORTED, "set_effectors: a pair (edge_fold) op must be last in the pipe");
        } else {
            n_entity_ops++;
        }
    }
    if (n_entity_ops > static_cast<size_t>(kMaxOps))
        return h->fail(SIXDOF_ERR_UNSUPPORTED, "set_effectors: at most 4 per-entity ops");
    if (n_pair > 1) return h->fail(SIXDOF_ERR_UNSUPPORTED, "set_effectors: at most one pair op");
    h->ops.assign(ops, ops + n_ops);
    h->replay.drop();
    return SIXDOF_OK;
} SIXDOF_ABI_CATCH(err_of(h))

int sixdof_set_edges(sixdof_handle* h, const uint64_t* from_ids, const uint64_t* to_ids, size_t n_edges) try {
    if (!h || ((!from_ids || !to_ids) && n_edges)) return SIXDOF_ERR_INVALID_ARGUMENT;
    if (!h->bound) return h->fail(SIXDOF_ERR_COMPONENT_NOT_FOUND, "set_edges: bind Body columns first");
    HIP_TRY(h, hipSetDevice(h->device));
    Edges ne;   // swapped in at the end: a failed call leaves the handle's edges as they were
    std::vector<uint32_t>&src = ne.src, &dst = ne.dst;
    const RowMap row_of = row_map(h->joined_ids);
    if (resolve_rows(row_of, from_ids, n_edges, &src) != n_edges || resolve_rows(row_of, to_ids, n_edges, &dst) != n_edges)
        return h->fail(SIXDOF_ERR_COMPONENT_NOT_FOUND, "set_edges: edge endpoint is not a Body entity");
    const uint32_t n = static_cast<uint32_t>(h->desc.n_entities);
    // CSR by source; a stable counting sort keeps each source's out-edges in spawn order, which is
    // the fold order of GraphQuery::edge_fold (graph.rs:113-175,239-361)
    std::vector<uint32_t> start(n + 1, 0), cdst(n_edges);
    for (size_t e = 0; e < n_edges; e++) start[src[e] + 1]++;
    for (uint32_t i = 0; i < n; i++) start[i + 1] += start[i];
    std::vector<uint32_t> cursor(start.begin(), start.end() - 1);
    for (size_t e = 0; e < n_edges; e++) cdst[cursor[src[e]]++] = dst[e];
    HIP_TRY(h, ne.d_csr_start.alloc((n + 1) * sizeof(uint32_t)));
    HIP_TRY(h, hipMemcpy(ne.d_csr_start.get(), start.data(), (n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (n_edges) {
        HIP_TRY(h, ne.d_csr_dst.alloc(n_edges * sizeof(uint32_t)));
        HIP_TRY(h, hipMemcpy(ne.d_csr_dst.get(), cdst.data(), n_edges * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    // hub sources: the fold kernels give them whole waves (pair_kernel.hpp 2c)
    std::vector<uint32_t> hub_rows, hub_chunk_start{0}, chunk_e0, chunk_row;
    const char* no_hubs = std::getenv("SIXDOF_NO_HUBS");   // A/B knob: "1" folds every source with one lane
    for (uint32_t i = 0; i < n && !(no_hubs && no_hubs[0] == '1'); i++) {
        const uint32_t deg = start[i + 1] - start[i];
        if (deg < kHubDegree) continue;
        hub_rows.push_back(i);
        for (uint32_t e = start[i]; e < start[i + 1]; e += kHubChunk) {
            chunk_e0.push_back(e);
            chunk_row.push_back(i);
        }
        hub_chunk_start.push_back(static_cast<uint32_t>(chunk_e0.size()));
    }
    ne.n_hubs = static_cast<uint32_t>(hub_rows.size());
    ne.n_hub_chunks = static_cast<uint32_t>(chunk_e0.size());
    if (ne.n_hubs) {
        std::vector<uint32_t> blob;
        blob.insert(blob.end(), hub_rows.begin(), hub_rows.end());
        blob.insert(blob.end(), hub_chunk_start.begin(), hub_chunk_start.end());
        blob.insert(blob.end(), chunk_e0.begin(), chunk_e0.end());
        blob.insert(blob.end(), chunk_row.begin(), chunk_row.end());
        HIP_TRY(h, ne.d_hub.alloc(blob.size() * sizeof(uint32_t)));
        HIP_TRY(h, hipMemcpy(ne.d_hub.get(), blob.data(), blob.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_TRY(h, ne.d_chunk_partial.alloc(static_cast<size_t>(ne.n_hub_chunks) * kPartialWidth * sizeof(double)));
    }
    std::swap(h->edges, ne);   // the previous tables are freed as `ne` goes
    h->replay.drop();
    return SIXDOF_OK;
} SIXDOF_ABI_CATCH(err_of(h))

int sixdof_get_join_rows(const sixdof_handle* h, uint64_t component_id, uint32_t* rows, size_t cap, size_t* n_out) try {
    if (!h || !n_out) return SIXDOF_ERR_INVALID_ARGUMENT;
    const Column* c = h->col(component_id);
    if (!c) return h->fail(SIXDOF_ERR_COMPONENT_NOT_FOUND, "get_join_rows: unknown component");
    const size_t m = h->joined_ids.size();
    *n_out = m;
    if (!rows) return SIXDOF_OK;
    if (cap < m) return h->fail(SIXDOF_ERR_VALUE_SIZE_MISMATCH, "get_join_rows: buffer too small");
    if (!c->joined) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, "get_join_rows: column is not part of the join yet");
    for (size_t j = 0; j < m; j++) rows[j] = c->rows.empty() ? static_cast<uint32_t>(j) : c->rows[j];
    return SIXDOF_OK;
} SIXDOF_ABI_CATCH(err_of(h))

int sixdof_get_edge_rows(const sixdof_handle* h, uint32_t* src_rows, uint32_t* dst_rows, size_t cap, size_t* n_out) try {
    if (!h || !n_out) return SIXDOF_ERR_INVALID_ARGUMENT;
    *n_out = h->edges.src.size();
    if (cap < h->edges.src.size()) return h->fail(SIXDOF_ERR_VALUE_SIZE_MISMATCH, "get_edge_rows: buffer too small");
    if (src_rows) std::memcpy(src_rows, h->edges.src.data(), h->edges.src.size() * sizeof(uint32_t));
    if (dst_rows) std::memcpy(dst_rows, h->edges.dst.data(), h->edges.dst.size() * sizeof(uint32_t));
    return SIXDOF_OK;
} SIXDOF_ABI_CATCH(err_of(h))

int prepare_graph(sixdof_handle* h);

int sixdof_upload(sixdof_handle* h) try {
    if (!h) return SIXDOF_ERR_INVALID_ARGUMENT;
    if (!h->bound) return h->fail(SIXDOF_ERR_COMPONENT_NOT_FOUND, "upload: no columns bound");
    HIP_TRY(h, hipSetDevice(h->device));
    const double t_up = now_ms();
    for (auto& kv : h->cols)
        if (int rc = upload_one(h, &kv.second); rc != SIXDOF_OK) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream.get()));
    h->last.h2d_upload_ms = now_ms() - t_up;
    h->resident = true;
    h->accel_is_host_data = true;
    return prepare_graph(h);   // SIXDOF_FLAG_USE_GRAPH: capture now, not inside the first long step call
} SIXDOF_ABI_CATCH(err_of(h))

// joined rows -> their places in the full column (before any D2H of that column)
static int scatter_back(sixdof_handle* h, Column* c) {
    if (c->joined && c->compact) {
        hipError_t e = launch_scatter_rows(c->dev.get(), c->compact.get(), c->d_rows.get<uint32_t>(), static_cast<uint32_t>(h->joined_ids.size()),
                                           static_cast<uint32_t>(c->width), c->elem, h->stream.get());
        if (e != hipSuccess) return h->hip_fail(e, "scatter_rows");
    }
    return SIXDOF_OK;
}

int sixdof_download(sixdof_handle* h, uint32_t mask) try {
    if (!h) return SIXDOF_ERR_INVALID_ARGUMENT;
    if (!h->bound) return h->fail(SIXDOF_ERR_COMPONENT_NOT_FOUND, "download: no columns bound");
    HIP_TRY(h, hipSetDevice(h->device));
    const double t_dn = now_ms();
    for (auto& b : h->body) {
        if (!(mask & b.bit)) continue;
        Column* c = h->col(b.id);
        if (!c) continue;
        int rc = scatter_back(h, c);
        if (rc != SIXDOF_OK) return rc;
        if (c->bytes) HIP_TRY(h, hipMemcpyAsync(c->host, c->dev.get(), c->bytes, hipMemcpyDeviceToHost, h->stream.get()));
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream.get()));
    h->last.d2h_download_ms = now_ms() - t_dn;
    return SIXDOF_OK;
} SIXDOF_ABI_CATCH(err_of(h))

int sixdof_download_async(sixdof_handle* h, uint32_t mask) try {
    if (!h) return SIXDOF_ERR_INVALID_ARGUMENT;
    if (!h->bound) return h->fail(SIXDOF_ERR_COMPONENT_NOT_FOUND, "download_async: no columns bound");
    HIP_TRY(h, hipSetDevice(h->device));
    CopyLane& lane = h->copy;
    HIP_TRY(h, lane.hold(h->stream.get()));   // the snapshot buffers are overwritten below
    Column* picked[5];
    int n_picked = 0;
    for (auto& b : h->body) {
        if (!(mask & b.bit)) continue;
        Column* c = h->col(b.id);
        if (!c || !c->bytes) continue;
        int rc = scatter_back(h, c);
        if (rc != SIXDOF_OK) return rc;
        if (!c->snap) HIP_TRY(h, c->snap.alloc(c->bytes));
        HIP_TRY(h, hipMemcpyAsync(c->snap.get(), c->dev.get(), c->bytes, hipMemcpyDeviceToDevice, h->stream.get()));
        if (!c->host_pinned) c->host_pinned.lock(c->host, c->bytes);   // once; an unlockable range is copied staged
        picked[n_picked++] = c;
    }
    HIP_TRY(h, lane.begin(h->stream.get()));
    for (int k = 0; k < n_picked; k++) HIP_TRY(h, lane.copy(picked[k]->host, picked[k]->snap.get(), picked[k]->bytes, 0));
    HIP_TRY(h, lane.end());
    return SIXDOF_OK;
} SIXDOF_ABI_CATCH(err_of(h))

int sixdof_download_wait(sixdof_handle* h) try {
    if (!h) return SIXDOF_ERR_INVALID_ARGUMENT;
    if (!h->copy.pending) return SIXDOF_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const double t0 = now_ms();
    HIP_TRY(h, hipEventSynchronize(h->copy.ev_copied.get()));
    h->copy.stream_lo = 1, h->copy.stream_hi = 0;   // every copy enqueued so far has landed: none reads the ring any more
    h->last.d2h_download_ms = now_ms() - t0;     // the part of the copy the host actually waited for
    return SIXDOF_OK;
} SIXDOF_ABI_CATCH(err_of(h))

int sixdof_sync(sixdof_handle* h) try {
    if (!h) return SIXDOF_ERR_INVALID_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream.get()));
    if (h->copy.stream) HIP_TRY(h, hipStreamSynchronize(h->copy.stream.get()));
    float ms0 = 0.f;
    if (h->step_pending && hipEventElapsedTime(&ms0, h->ev0.get(), h->ev1.get()) == hipSuccess) h->last.kernel_device_ms = ms0;
    h->step_pending = h->prev_pending = false;
    h->copy.pending = false;
    h->copy.stream_lo = 1, h->copy.stream_hi = 0;
    // page locks taken on the caller's history buffers end here: the caller may free them after sixdof_sync
    h->copy.pinned_user.clear();
    return SIXDOF_OK;
} SIXDOF_ABI_CATCH(err_of(h))

int sixdof_get_tick(const sixdof_handle* h, uint64_t* tick) try {
    if (!h || !tick) return SIXDOF_ERR_INVALID_ARGUMENT;
    *tick = h->tick;
    return SIXDOF_OK;
} SIXDOF_ABI_CATCH(err_of(h))
int sixdof_set_tick(sixdof_handle* h, uint64_t tick) try {
    if (!h) return SIXDOF_ERR_INVALID_ARGUMENT;
    h->tick = tick;
    h->hist.first_tick = tick + 1;
    return SIXDOF_OK;
} SIXDOF_ABI_CATCH(err_of(h))
int sixdof_set_ticks_per_launch(sixdof_handle* h, uint32_t k) try {
    if (!h || k == 0) return SIXDOF_ERR_INVALID_ARGUMENT;
    h->desc.ticks_per_launch = k;
    h->replay.drop();
    return h->resident ? prepare_graph(h) : SIXDOF_OK;
} SIXDOF_ABI_CATCH(err_of(h))

int sixdof_set_flags(sixdof_handle* h, uint32_t flags) try {
    if (!h) return SIXDOF_ERR_INVALID_ARGUMENT;
    h->desc.flags = flags;
    return SIXDOF_OK;
} SIXDOF_ABI_CATCH(err_of(h))

void* sixdof_device_column(sixdof_handle* h, uint64_t component_id) try {
    if (!h) return nullptr;
    Column* c = h->col(component_id);
    return c ? (c->live ? c->live : c->dev.get()) : nullptr;
} SIXDOF_ABI_CATCH_VALUE(err_of(h), nullptr)
void* sixdof_stream(sixdof_handle* h) { return h ? static_cast<void*>(h->stream.get()) : nullptr; }

}  // extern "C"

// ---- step --------------------------------------------------------------------------------------------------

namespace {

int build_dev_ops(sixdof_handle* h, DevOp* out, uint32_t* n_out, uint32_t* vel_independent) {
    uint32_t n = 0;
    *vel_independent = 1;
    if (h->custom_launch) {   // generated pipe: slots are just the columns its code reads
        for (size_t k = 0; k < h->custom_folds.size(); k++)
            if (h->custom_folds[k].needs_table && !h->custom_folds[k].set)
                return h->fail(SIXDOF_ERR_UNSUPPORTED, "step: fold stage " + std::to_string(k) + " of the installed program reads its edges from "
                               "device memory and has no table yet (sixdof_set_fold_edges)");
        for (uint64_t id : h->custom_aux) {
            Column* c = h->col(id);
            if (!c) return h->fail(SIXDOF_ERR_COMPONENT_NOT_FOUND, "step: column read by the generated pipe is not bound");
            if (c->width < 1 || c->width > 3 || c->prim != h->state_prim())
                return h->fail(SIXDOF_ERR_VALUE_SIZE_MISMATCH, "step: generated-pipe columns must be [n,1..3] of the state dtype");
            if (int rc = ensure_joined(h, c); rc != SIXDOF_OK) return rc;
            DevOp d{};
            d.aux = c->live;
            d.aux_width = static_cast<int32_t>(c->width);
            out[n++] = d;
        }
        *n_out = n;
        return SIXDOF_OK;
    }
    for (auto& o : h->ops) {
        if (SIXDOF_EFF_IS_PAIR(o.kind)) continue;
        DevOp d{};
        d.kind = o.kind;
        std::memcpy(d.p, o.p, sizeof(d.p));
        if (o.kind == SIXDOF_EFF_BODY_TORQUE || o.kind == SIXDOF_EFF_BODY_FORCE || o.kind == SIXDOF_EFF_BALL_DRAG ||
            o.kind == SIXDOF_EFF_WORLD_TORQUE || o.kind == SIXDOF_EFF_WORLD_FORCE) {
            Column* c = h->col(o.aux_component_id);
            if (!c) return h->fail(SIXDOF_ERR_COMPONENT_NOT_FOUND, "step: effector aux column not bound");
            // the built-in kernels count on this refusal: they load [n,3] rows with the width fixed at compile time and most of
            // them never read DevOp::aux_width, which stays 0 here (step_kernel.hpp, kAuxRows3)
            if (c->width != 3 || c->prim != h->state_prim())
                return h->fail(SIXDOF_ERR_VALUE_SIZE_MISMATCH, "step: effector aux column must be [n,3] of the state dtype");
            if (int rc = ensure_joined(h, c); rc != SIXDOF_OK) return rc;
            d.aux = c->live;
        }
        if (o.kind == SIXDOF_EFF_BALL_DRAG) *vel_independent = 0;
        out[n++] = d;
    }
    *n_out = n;
    return SIXDOF_OK;
}

int fill_step_params(sixdof_handle* h, StepParams* P) {
    std::memset(P, 0, sizeof(*P));
    P->pos = h->col(h->id_pos)->live;
    P->vel = h->col(h->id_vel)->live;
    P->accel = h->col(h->id_accel)->live;
    P->force = h->col(h->id_force)->live;
    P->inertia = h->col(h->id_inertia)->live;
    P->n = static_cast<uint32_t>(h->desc.n_entities);
    P->dt_g = h->desc.simulation_time_step;
    P->dt = h->desc.has_time_step ? h->desc.time_step : h->desc.simulation_time_step;
    // Cache policy of the launch (step_kernel.hpp: load * 8 + store, bit 8 = one flush after the tick instead of columns
    // stored as they complete), by working-set size, from the A/B matrices in profiles/r02_step_ab_load_x_store_policy.txt
    // and r02_step_ab_policy_by_size.txt (f64 body counts in brackets):
    //   <= 768 MiB [<= 3.1M]      plain loads, nt stores, early     65,536: 5.48 -> 4.93 us   262,144: 16.6 -> 16.3 us
    //                                                               1,048,576: 61.9 -> 60.0   2,097,152: 136 -> 123 us
    //   beyond                    nt loads,    nt stores, early     4,194,304: 300 -> 263 us
    // (inputs are re-read next tick: keep them cacheable while the 256 MiB Infinity Cache can hold them; outputs are
    // written once per tick: never worth a line).  SIXDOF_STREAMING=<code> overrides it for A/B runs (tools/step_ab.py).
    const char* force_nt = std::getenv("SIXDOF_STREAMING");
    size_t row_elems = 32;      // the Body columns: pos 7 + vel 6 + accel 6 + force 6 + inertia 7
    for (size_t k = 0; k < h->custom_model.size(); k++)      // + the component columns of a generated program (Falcon 9: 201 values)
        if (const Column* c = h->col(h->custom_model[k])) row_elems += c->width;
    const size_t state_bytes = static_cast<size_t>(h->desc.n_entities) * row_elems * h->elem_size();
    // NOT the write-through (`sc1`) store policy, although it measured 7 % faster between 48 and 192 MiB of state: the next
    // launch can read STALE rows after it (262,144 bodies: ~10 % of the rows differ from the fused run, differently every
    // run — tools/debug_midsize_determinism.py, profiles/r02_sc1_store_policy_is_unsafe.txt).  It is compiled into the A/B
    // library only (`make ab`, -DSIXDOF_AB_BUILD); the product ignores any SIXDOF_STREAMING code outside {0, 1, 9}.
    uint32_t policy = 9u;
    if (state_bytes <= (768ull << 20)) policy = 1u;
    if (force_nt) {
        const uint32_t code = static_cast<uint32_t>(std::atoi(force_nt));
#ifdef SIXDOF_AB_BUILD
        policy = code;
#else
        // the product library carries the three safe policies only (plain / nt stores / nt both ways, + the late-flush bit)
        const uint32_t pol = code & 255u;
        if ((code & ~0x1ffu) == 0 && (pol == 0u || pol == 1u || pol == 9u)) policy = code;
#endif
    }
    P->streaming = policy;
    P->hist_ring = h->hist.ring;
    if (h->hist.ring) {
        P->hist_pos = h->hist.body[0].get();
        P->hist_vel = h->hist.body[1].get();
        P->hist_accel = h->hist.body[2].get();
        P->hist_force = h->hist.body[3].get();
    }
    for (size_t k = 0; k < h->custom_model.size(); k++) {
        Column* c = h->col(h->custom_model[k]);
        if (!c) return h->fail(SIXDOF_ERR_COMPONENT_NOT_FOUND, "step: component column of the generated program is not bound");
        const unsigned expect = k < h->custom_model_width.size() ? h->custom_model_width[k] : 0u;
        const bool window = (expect >> 31) != 0;
        const size_t want = expect & 0x1fffffffu;     // bit 30: built for the element-major window layout; bit 29: element-major register columns
        if (c->prim != h->state_prim() || c->width < 1 || (!window && c->width > 64) || (want && c->width != want))
            return h->fail(SIXDOF_ERR_VALUE_SIZE_MISMATCH,
                           "step: program columns must be of the state dtype and as wide as the generated code expects "
                           "([n,1..64]; a window column [n, rows*width])");
        if (!c->joined) {
            int rc = resolve_join(h, c);
            if (rc != SIXDOF_OK) return rc;
            if (c->compact && ((expect >> 29) & 1u))      // the gather / scatter kernels move [n,w] rows
                return h->fail(SIXDOF_ERR_UNSUPPORTED, "step: a program built for element-major columns needs every column on "
                                                       "the executor's own entity set (no entity-set join)");
            if (rc = gather_joined(h, c); rc != SIXDOF_OK) return rc;
        }
        P->model_cols[k] = c->live;
        P->model_hist[k] = (h->hist.ring && k < h->hist.model.size()) ? h->hist.model[k].get() : nullptr;
    }
    P->tick0 = h->tick;
    return build_dev_ops(h, P->ops, &P->n_ops, &P->vel_independent);
}

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// built-in pipes or the handle's generated pipe
hipError_t launch_any(sixdof_handle* h, const StepParams& P) {
    if (h->desc.integrator == SIXDOF_INTEGRATOR_NONE && !h->custom_launch) return hipErrorInvalidValue;
    if (h->custom_launch) {
        // the object keeps the tables it launches with per thread (one object may serve several handles): hand this handle's over
        for (size_t k = 0; k < h->custom_folds.size(); k++)
            if (h->custom_folds[k].needs_table) h->custom_set_fold_table(static_cast<unsigned>(k), h->custom_folds[k].set ? &h->custom_folds[k].table : nullptr);
        return static_cast<hipError_t>(h->custom_launch(&P, h->desc.integrator, h->desc.dtype, h->stream.get()));
    }
    return launch_step(P, h->desc.integrator, h->desc.dtype, h->stream.get());
}

int fill_pair_params(sixdof_handle* h, PairParams* P) {
    std::memset(P, 0, sizeof(*P));
    const size_t n = h->desc.n_entities;
    const size_t es = h->elem_size();
    const sixdof_effector_op& pop = h->ops.back();
    const uint32_t splits = pop.kind == SIXDOF_EFF_ALLPAIRS_GRAVITY_SOFTENED ? pair_splits_for(static_cast<uint32_t>(n)) : 1;
    (void)es;
    // scratch layout: pack[n,10] | partial[splits,n,width]   (f64)
    const bool allpairs = pop.kind == SIXDOF_EFF_ALLPAIRS_GRAVITY_SOFTENED;
    const size_t pwidth = allpairs ? kPartialForce : kPartialWidth;
    const size_t pack_bytes = align_up(sizeof(double) * kPackWidth * n, 256);
    const size_t partial_bytes = align_up(sizeof(double) * pwidth * n * splits, 256);
    const size_t total = pack_bytes + partial_bytes + (allpairs ? 0 : pack_bytes);      // edge lists: a second pack buffer (the one-launch tick ping-pongs)
    if (total > h->d_scratch.bytes()) HIP_TRY(h, h->d_scratch.alloc(total));   // free first; on failure empty
    char* base = h->d_scratch.get<char>();
    P->pos = h->col(h->id_pos)->live;
    P->vel = h->col(h->id_vel)->live;
    P->accel = h->col(h->id_accel)->live;
    P->force = h->col(h->id_force)->live;
    P->inertia = h->col(h->id_inertia)->live;
    P->n = static_cast<uint32_t>(n);
    P->dt_g = h->desc.simulation_time_step;
    P->dt = h->desc.has_time_step ? h->desc.time_step : h->desc.simulation_time_step;
    P->pack = reinterpret_cast<double*>(base);
    P->partial = reinterpret_cast<double*>(base + pack_bytes);
    P->pack_next = allpairs ? nullptr : reinterpret_cast<double*>(base + pack_bytes + partial_bytes);
    P->splits = splits;
    P->partial_width = static_cast<uint32_t>(pwidth);
    P->pair_kind = pop.kind;
    P->p0 = pop.p[0];
    P->p1 = pop.p[1];
    if (pop.kind != SIXDOF_EFF_ALLPAIRS_GRAVITY_SOFTENED) {
        const Edges& ed = h->edges;
        if (!ed.d_csr_start) return h->fail(SIXDOF_ERR_COMPONENT_NOT_FOUND, "step: edge effector without sixdof_set_edges");
        P->row_start = ed.d_csr_start.get<uint32_t>();
        P->dst = ed.d_csr_dst.get<uint32_t>();
        P->n_edges = static_cast<uint32_t>(ed.src.size());
        P->n_hubs = ed.n_hubs;
        P->n_hub_chunks = ed.n_hub_chunks;
        if (ed.n_hubs) {
            P->hub_rows = ed.d_hub.get<uint32_t>();
            P->hub_chunk_start = P->hub_rows + ed.n_hubs;
            P->chunk_e0 = P->hub_chunk_start + (ed.n_hubs + 1);
            P->chunk_row = P->chunk_e0 + ed.n_hub_chunks;
            P->chunk_partial = ed.d_chunk_partial.get<double>();
        }
    }
    uint32_t vi = 0;
    return build_dev_ops(h, P->ops, &P->n_ops, &vi);
}

// reference.py:164-175 (bisect_right interpolation), evaluated once per tick on the host: every rollout
// of a campaign sees the same reference profile at a given tick.
double ref_interp(double t, const std::vector<double>& xs, const std::vector<double>& ys) {
    const size_t n = xs.size();
    if (t <= xs[0]) return ys[0];
    if (t >= xs[n - 1]) return ys[n - 1];
    size_t lo = 0, hi = n;
    while (lo < hi) {
        const size_t mid = (lo + hi) / 2;
        if (t < xs[mid]) hi = mid; else lo = mid + 1;
    }
    const size_t a = lo - 1, b = lo;
    const double span = xs[b] - xs[a];
    if (span <= 0.0) return ys[a];
    const double frac = (t - xs[a]) / span;
    return ys[a] + (ys[b] - ys[a]) * frac;
}

// Telemetry ring for the paths whose kernels do not record in-line (pair / edge_fold ticks, the Apollo model): with a
// ring enabled those paths are stepped ONE tick per launch and the four live output columns are copied, device to
// device on the compute stream, into the tick's ring slot — every tick is there, in the layout sixdof_history_read /
// _stream expect.  (The fused per-entity kernel records from registers instead, step_kernel.hpp.)
int snapshot_tick_to_ring(sixdof_handle* h, uint64_t ticks_done) {
    if (!h->hist.ring) return SIXDOF_OK;
    const size_t n = h->desc.n_entities, es = h->elem_size();
    const size_t slot = static_cast<size_t>(history_slot(ticks_done, h->hist.ring));
    for (int k = 0; k < 4; k++) {
        const size_t block = n * h->body[k].width * es;
        if (!block) continue;
        HIP_TRY(h, hipMemcpyAsync(h->hist.body[k].get<char>() + slot * block, h->col(h->body[k].id)->live, block,
                                  hipMemcpyDeviceToDevice, h->stream.get()));
    }
    return SIXDOF_OK;
}

int step_apollo(sixdof_handle* h, uint64_t n_ticks, uint64_t* launches) {
    const char* names[5] = {"apollo_state", "apollo_params", "apollo_guidance", "apollo_score", "apollo_result"};
    const uint64_t widths[5] = {APOLLO_N_STATE, APOLLO_N_PARAMS, APOLLO_N_GUIDANCE, APOLLO_N_SCORE, APOLLO_N_RESULT};
    Column* c[5];
    for (int k = 0; k < 5; k++) {
        c[k] = h->col(cid(names[k]));
        if (!c[k]) return h->fail(SIXDOF_ERR_COMPONENT_NOT_FOUND, std::string("step: Apollo model column not bound: ") + names[k]);
        if (c[k]->width != widths[k] || c[k]->prim != SIXDOF_PRIM_F64)
            return h->fail(SIXDOF_ERR_VALUE_SIZE_MISMATCH, std::string("step: bad shape for ") + names[k]);
        if (int rc = ensure_joined(h, c[k]); rc != SIXDOF_OK) return rc;
    }
    ApolloParams P{};
    P.pos = static_cast<double*>(h->col(h->id_pos)->live);
    P.vel = static_cast<double*>(h->col(h->id_vel)->live);
    P.accel = static_cast<double*>(h->col(h->id_accel)->live);
    P.force = static_cast<double*>(h->col(h->id_force)->live);
    P.inertia = static_cast<double*>(h->col(h->id_inertia)->live);
    P.state = static_cast<double*>(c[0]->live);
    P.params = static_cast<const double*>(c[1]->live);
    P.guidance = static_cast<double*>(c[2]->live);
    P.score = static_cast<double*>(c[3]->live);
    P.result = static_cast<double*>(c[4]->live);
    P.n = static_cast<uint32_t>(h->desc.n_entities);
    P.max_ticks = h->ap_max_ticks;
    P.guidance_period = h->ap_guidance_period;
    P.ticks_per_telemetry = h->ap_ticks_per_telemetry;
    P.dt = h->desc.simulation_time_step;
    const uint32_t K = h->hist.ring ? 1u : h->desc.ticks_per_launch;   // recording: one tick per launch, see snapshot_tick_to_ring
    if (const size_t need = static_cast<size_t>(K) * 8 * sizeof(double); need > h->d_tick_refs.bytes())
        HIP_TRY(h, h->d_tick_refs.alloc(need));   // free first; on failure empty
    std::vector<double> refs(static_cast<size_t>(K) * 8);
    uint64_t done = 0;
    while (done < n_ticks) {
        const uint32_t k = static_cast<uint32_t>(std::min<uint64_t>(K, n_ticks - done));
        for (uint32_t j = 0; j < k; j++) {
            // post_step's t_s = end_tick * SIM_TIME_STEP with end_tick = ticks completed - 1 (impeller2_server.rs:566,671)
            const double t_s = static_cast<double>(h->tick + done + j) * (1.0 / 120.0);
            double* r = &refs[static_cast<size_t>(j) * 8];
            r[0] = ref_interp(t_s, h->ap_time, h->ap_alt);
            r[1] = ref_interp(t_s, h->ap_time, h->ap_rate);
            r[2] = std::fabs(ref_interp(t_s, h->ap_time, h->ap_pitch));
            r[3] = ref_interp(t_s, h->ap_time, h->ap_hspeed);
            r[4] = ref_interp(t_s, h->ap_time, h->ap_downrange);
            r[5] = r[3] - ref_interp(t_s + 1.0, h->ap_time, h->ap_hspeed);
            r[6] = r[7] = 0.0;
        }
        // stream-ordered: the previous launch has consumed the buffer before this copy executes
        HIP_TRY(h, hipMemcpyAsync(h->d_tick_refs.get(), refs.data(), static_cast<size_t>(k) * 8 * sizeof(double),
                                  hipMemcpyHostToDevice, h->stream.get()));
        HIP_TRY(h, hipStreamSynchronize(h->stream.get()));  // `refs` is reused by the next chunk
        P.tick_refs = h->d_tick_refs.get<double>();
        P.n_ticks = k;
        P.tick0 = h->tick + done;
        hipError_t e = launch_apollo(P, h->stream.get());
        if (e != hipSuccess) return h->hip_fail(e, "launch_apollo");
        (*launches)++;
        done += k;
        if (h->hist.ring) {
            int rc = snapshot_tick_to_ring(h, h->tick + done);
            if (rc != SIXDOF_OK) return rc;
        }
    }
    return SIXDOF_OK;
}

}  // namespace

extern "C" {

int sixdof_set_model_apollo(sixdof_handle* h, const sixdof_apollo_tables* t) try {
    if (!h || !t || t->n < 2 || !t->time_s || !t->altitude_m || !t->descent_rate_mps || !t->pitch_deg ||
        !t->horizontal_speed_mps || !t->downrange_m)
        return SIXDOF_ERR_INVALID_ARGUMENT;
    if (h->desc.integrator != SIXDOF_INTEGRATOR_SEMI_IMPLICIT || h->desc.dtype != SIXDOF_F64)
        return h->fail(SIXDOF_ERR_UNSUPPORTED, "set_model_apollo: the example uses el.Integrator.SemiImplicit in f64 (sim.py:523)");
    h->ap_time.assign(t->time_s, t->time_s + t->n);
    h->ap_alt.assign(t->altitude_m, t->altitude_m + t->n);
    h->ap_rate.assign(t->descent_rate_mps, t->descent_rate_mps + t->n);
    h->ap_pitch.assign(t->pitch_deg, t->pitch_deg + t->n);
    h->ap_hspeed.assign(t->horizontal_speed_mps, t->horizontal_speed_mps + t->n);
    h->ap_downrange.assign(t->downrange_m, t->downrange_m + t->n);
    h->ap_guidance_period = t->guidance_period_ticks ? t->guidance_period_ticks : 5;
    h->ap_ticks_per_telemetry = t->ticks_per_telemetry ? t->ticks_per_telemetry : 3;
    h->ap_max_ticks = t->max_ticks;
    h->model = 1;
    return SIXDOF_OK;
} SIXDOF_ABI_CATCH(err_of(h))

int sixdof_last_timings(const sixdof_handle* h, sixdof_timings* out) try {
    if (!h || !out) return SIXDOF_ERR_INVALID_ARGUMENT;
    *out = h->last;
    return SIXDOF_OK;
} SIXDOF_ABI_CATCH(err_of(h))

int sixdof_count_nonfinite(sixdof_handle* h, uint64_t* count, uint8_t* row_flags) try {
    if (!h || !count) return SIXDOF_ERR_INVALID_ARGUMENT;
    if (!h->bound) return h->fail(SIXDOF_ERR_COMPONENT_NOT_FOUND, "count_nonfinite: no columns bound");
    HIP_TRY(h, hipSetDevice(h->device));
    const uint32_t n = static_cast<uint32_t>(h->desc.n_entities);
    DeviceBuffer d_count, d_flags;
    HIP_TRY(h, d_count.alloc(sizeof(unsigned long long)));
    hipError_t e = hipMemsetAsync(d_count.get(), 0, sizeof(unsigned long long), h->stream.get());
    if (e == hipSuccess && row_flags && n) e = d_flags.alloc(n);
    if (e == hipSuccess)
        e = launch_nonfinite(h->col(h->id_pos)->live, h->col(h->id_vel)->live, n, h->elem_size(), d_flags.get<uint8_t>(),
                             d_count.get<unsigned long long>(), h->stream.get());
    unsigned long long host_count = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&host_count, d_count.get(), sizeof(host_count), hipMemcpyDeviceToHost, h->stream.get());
    if (e == hipSuccess && d_flags) e = hipMemcpyAsync(row_flags, d_flags.get(), n, hipMemcpyDeviceToHost, h->stream.get());
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream.get());
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(h->stream.get());   // what was enqueued names host_count and the two buffers: it must not outlive them
        return h->hip_fail(e, "count_nonfinite");
    }
    *count = host_count;
    return SIXDOF_OK;
} SIXDOF_ABI_CATCH(err_of(h))

int sixdof_set_custom_pipe(sixdof_handle* h, const char* so_path, const uint64_t* aux_ids, size_t n_aux) try {
    if (!h || !so_path || (!aux_ids && n_aux)) return SIXDOF_ERR_INVALID_ARGUMENT;
    DlHandle owned;   // closed again by every early return
    void* dl = *owned.out() = dlopen(so_path, RTLD_NOW | RTLD_LOCAL);
    if (!dl) return h->fail(SIXDOF_ERR_BACKEND, std::string("set_custom_pipe: dlopen failed: ") + dlerror());
    auto abi = reinterpret_cast<CustomAbiFn>(dlsym(dl, "sixdof_custom_abi"));
    auto layout = reinterpret_cast<CustomLayoutFn>(dlsym(dl, "sixdof_custom_layout"));
    auto launch = reinterpret_cast<CustomLaunchFn>(dlsym(dl, "sixdof_custom_launch"));
    if (!abi || !layout || !launch || abi() != sizeof(StepParams))
        return h->fail(SIXDOF_ERR_BACKEND, "set_custom_pipe: not a generated pipe for this library build (StepParams layout differs)");
    auto col_widths = reinterpret_cast<void (*)(unsigned*)>(dlsym(dl, "sixdof_custom_column_widths"));
    // a program that exchanges data between the entities of a world inside the wavefront (a whole-world StableHLO tick with one lane
    // per entity: elodin_amd/stablehlo.py, manifest "rows_per_world") lays a world out as that many consecutive rows
    auto rows_multiple = reinterpret_cast<unsigned (*)()>(dlsym(dl, "sixdof_custom_rows_multiple"));
    if (rows_multiple && rows_multiple() > 1 && h->desc.n_entities % rows_multiple() != 0)
        return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, "set_custom_pipe: the program lays a world out as " + std::to_string(rows_multiple()) +
                       " consecutive rows; " + std::to_string(h->desc.n_entities) + " rows are not a whole number of worlds");
    const unsigned lay = layout();
    const size_t k_aux = lay & 0xff, k_model = (lay >> 8) & 0xff;
    if (k_aux > static_cast<size_t>(kMaxOps) || k_model > static_cast<size_t>(kMaxModelCols) || k_aux + k_model != n_aux)
        return h->fail(SIXDOF_ERR_VALUE_SIZE_MISMATCH, "set_custom_pipe: column list does not match the generated code's layout");
    // fold stages that read their edges from device memory (optional exports; an object without them bakes its edges)
    auto fold_count = reinterpret_cast<unsigned (*)()>(dlsym(dl, "sixdof_custom_fold_count"));
    auto fold_info = reinterpret_cast<int (*)(unsigned, unsigned*)>(dlsym(dl, "sixdof_custom_fold_info"));
    auto set_fold_table = reinterpret_cast<SetFoldTableFn>(dlsym(dl, "sixdof_custom_set_fold_table"));
    std::vector<FoldSlot> folds;
    if (fold_count && fold_info && set_fold_table) {
        folds.resize(fold_count());
        for (size_t k = 0; k < folds.size(); k++) {
            unsigned info[4] = {0, 0, 0, 0};
            if (fold_info(static_cast<unsigned>(k), info) != 0 || info[3] != sizeof(FoldTable))
                return h->fail(SIXDOF_ERR_BACKEND, "set_custom_pipe: the object's fold tables are not this library build's (FoldTable layout differs)");
            folds[k].needs_table = (info[0] & 1u) != 0;
            folds[k].wave_ok = (info[0] & 2u) != 0;
            folds[k].count = info[1];
            folds[k].stride = info[2];
        }
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream.get()));      // nothing in flight reads the tables of the program being replaced
    h->custom_set_fold_table = folds.empty() ? nullptr : set_fold_table;
    h->custom_folds = std::move(folds);   // frees the previous program's tables
    h->custom_dl = std::move(owned);      // and closes its object
    h->custom_launch = launch;
    h->custom_rows_multiple = rows_multiple ? rows_multiple() : 1;      // checked again when the join is (re)sized: sixdof_bind_columns
    h->custom_aux.assign(aux_ids, aux_ids + k_aux);
    h->custom_model.assign(aux_ids + k_aux, aux_ids + k_aux + k_model);
    h->custom_tick_free = ((lay >> 17) & 1u) != 0;
    // row widths the generated code was built for (bit 31: a window column — memory-resident, any width, not recorded)
    h->custom_model_width.assign(k_model, 0u);
    if (col_widths && k_model) col_widths(h->custom_model_width.data());
    h->ops.clear();
    h->replay.drop();
    return SIXDOF_OK;
} SIXDOF_ABI_CATCH(err_of(h))

int sixdof_set_fold_edges(sixdof_handle* h, uint32_t fold_index, const uint64_t* from_ids, const uint64_t* to_ids, size_t n_edges) try {
    if (!h || ((!from_ids || !to_ids) && n_edges)) return SIXDOF_ERR_INVALID_ARGUMENT;
    if (!h->custom_launch) return h->fail(SIXDOF_ERR_UNSUPPORTED, "set_fold_edges: no generated program is installed (sixdof_set_custom_pipe)");
    if (!h->custom_set_fold_table)
        return h->fail(SIXDOF_ERR_UNSUPPORTED, "set_fold_edges: the installed program bakes its folds' edges into its code; build it with device fold tables");
    if (fold_index >= h->custom_folds.size())
        return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, "set_fold_edges: fold_index " + std::to_string(fold_index) + " out of range (the program has " +
                       std::to_string(h->custom_folds.size()) + " fold stages)");
    FoldSlot& f = h->custom_folds[fold_index];
    if (!f.needs_table) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, "set_fold_edges: this fold stage folds the complete graph of a world: it has no edge table");
    if (!h->bound) return h->fail(SIXDOF_ERR_COMPONENT_NOT_FOUND, "set_fold_edges: bind Body columns first");
    if (n_edges > 0xFFFFFFFFull) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, "set_fold_edges: more than 2^32 - 1 edges");
    const uint64_t n = h->desc.n_entities;
    const bool replicated = f.count > 1 || f.stride > 0;
    if (replicated && static_cast<uint64_t>(f.count) * f.stride != n)
        return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, "set_fold_edges: the program was generated for " + std::to_string(f.count) + " replicas of " +
                       std::to_string(f.stride) + " rows; the handle has " + std::to_string(n) + " rows");
    const uint32_t row_limit = replicated ? f.stride : static_cast<uint32_t>(std::min<uint64_t>(n, 0xFFFFFFFFull));
    std::vector<uint32_t> src, dst;
    const RowMap row_of = row_map(h->joined_ids);
    if (resolve_rows(row_of, from_ids, n_edges, &src) != n_edges || resolve_rows(row_of, to_ids, n_edges, &dst) != n_edges)
        return h->fail(SIXDOF_ERR_COMPONENT_NOT_FOUND, "set_fold_edges: edge endpoint is not an entity of this handle");
    // one block [src_rows (n_src) | row_start (n_src + 1) | dst (n_edges)], built for the most sources there can be
    std::vector<uint32_t> o_src(n_edges), o_start(n_edges + 1), o_dst(n_edges);
    uint32_t n_src = 0, n_lane = 0;
    const int brc = sixdof_build_fold_table(src.data(), dst.data(), n_edges, row_limit, f.wave_ok ? kFoldWaveDegree : 0u, o_src.data(),
                                            o_start.data(), o_dst.data(), &n_src, &n_lane);
    if (brc == SIXDOF_ERR_INVALID_ARGUMENT)
        return h->fail(brc, replicated ? "set_fold_edges: with replicas the edges name entities of replica 0 only" : "set_fold_edges: an edge row lies outside the handle's rows");
    if (brc != SIXDOF_OK) return h->fail(brc, "set_fold_edges: the table could not be built (out of memory)");
    std::vector<uint32_t> blob;
    blob.reserve(static_cast<size_t>(n_src) * 2 + 1 + n_edges);
    blob.insert(blob.end(), o_src.begin(), o_src.begin() + n_src);
    blob.insert(blob.end(), o_start.begin(), o_start.begin() + n_src + 1);
    blob.insert(blob.end(), o_dst.begin(), o_dst.end());
    HIP_TRY(h, hipSetDevice(h->device));
    DeviceBuffer fresh;
    HIP_TRY(h, fresh.alloc(blob.size() * sizeof(uint32_t)));
    hipError_t e = hipMemcpyAsync(fresh.get(), blob.data(), blob.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream.get());
    // drains the batches that still read the old table, and the copy itself (its source is a local)
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream.get());
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(h->stream.get());   // a copy that was enqueued names `blob` and `fresh`: it must not outlive them
        return h->hip_fail(e, "set_fold_edges: upload");
    }
    f.d_blob = std::move(fresh);
    const uint32_t* d_new = f.d_blob.get<uint32_t>();
    f.table.src_rows = d_new;
    f.table.row_start = d_new + n_src;
    f.table.dst = d_new + static_cast<size_t>(n_src) * 2 + 1;
    f.table.n_src = n_src;
    f.table.n_lane = n_lane;
    f.set = true;
    h->replay.drop();      // captured launches hold the old pointers and grid sizes
    return SIXDOF_OK;
} SIXDOF_ABI_CATCH(err_of(h))

int sixdof_set_custom_pair(sixdof_handle* h, const char* so_path) try {
    if (!h || !so_path) return SIXDOF_ERR_INVALID_ARGUMENT;
    if (h->custom_launch) return h->fail(SIXDOF_ERR_UNSUPPORTED, "set_custom_pair: a generated per-entity pipe is installed; pair folds combine with built-in ops only");
    DlHandle owned;
    void* dl = *owned.out() = dlopen(so_path, RTLD_NOW | RTLD_LOCAL);
    if (!dl) return h->fail(SIXDOF_ERR_BACKEND, std::string("set_custom_pair: dlopen failed: ") + dlerror());
    auto abi = reinterpret_cast<CustomPairAbiFn>(dlsym(dl, "sixdof_custom_pair_abi"));
    auto launch = reinterpret_cast<CustomPairLaunchFn>(dlsym(dl, "sixdof_custom_pair_launch"));
    if (!abi || !launch || abi() != sizeof(PairParams))
        return h->fail(SIXDOF_ERR_BACKEND, "set_custom_pair: not a generated pair fold for this library build (PairParams layout differs)");
    h->pair_dl = std::move(owned);   // closes the previous object
    h->pair_launch = launch;
    // an object generated for one launch shape only (codegen.build_pair(small=...)) says which: step follows the object
    auto only_small = reinterpret_cast<int (*)()>(dlsym(dl, "sixdof_custom_pair_only_small"));
    h->pair_only_small = only_small ? only_small() : -1;
    while (!h->ops.empty() && SIXDOF_EFF_IS_PAIR(h->ops.back().kind)) h->ops.pop_back();
    sixdof_effector_op op{};
    op.kind = SIXDOF_EFF_EDGE_CUSTOM;
    h->ops.push_back(op);
    h->replay.drop();
    return SIXDOF_OK;
} SIXDOF_ABI_CATCH(err_of(h))

// Column m of the installed program if the ring records it, else null: a window column is its own history (and far too wide
// to copy per tick), an unbound one has nothing to record.
static const Column* recorded_model_column(const sixdof_handle* h, size_t m) {
    const bool window = m < h->custom_model_width.size() && (h->custom_model_width[m] >> 31);
    return window ? nullptr : h->col(h->custom_model[m]);
}

int sixdof_set_history(sixdof_handle* h, uint32_t ring_ticks) try {
    if (!h) return SIXDOF_ERR_INVALID_ARGUMENT;
    if (!h->bound) return h->fail(SIXDOF_ERR_COMPONENT_NOT_FOUND, "set_history: bind Body columns first");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream.get()));
    // the copy stream may still read the ring (sixdof_history_stream) or a staging buffer that lives with it (the reductions, the scans)
    if (h->copy.pending) {
        HIP_TRY(h, hipStreamSynchronize(h->copy.stream.get()));
        h->copy.stream_lo = 1, h->copy.stream_hi = 0;
    }
    h->hist.reset();   // free first (rings can be gigabytes): from here to the end of a successful call there is no ring
    h->replay.drop();
    if (ring_ticks == 0) return SIXDOF_OK;
    History fresh;     // freed as a whole by any failure below
    auto alloc_ring = [&](DeviceBuffer& ring, uint64_t width) {
        const size_t bytes = static_cast<size_t>(ring_ticks) * h->desc.n_entities * width * h->elem_size();
        return ring.alloc(bytes ? bytes : 16);
    };
    for (int k = 0; k < 4; k++)
        if (hipError_t e = alloc_ring(fresh.body[k], h->body[k].width); e != hipSuccess) return h->hip_fail(e, "set_history: hipMalloc of the ring");
    fresh.model.resize(h->custom_model.size());
    for (size_t m = 0; m < h->custom_model.size(); m++)      // component columns of a generated program are recorded too
        if (const Column* c = recorded_model_column(h, m))
            if (hipError_t e = alloc_ring(fresh.model[m], c->width); e != hipSuccess) return h->hip_fail(e, "set_history: hipMalloc of a component ring");
    fresh.ring = ring_ticks;
    fresh.first_tick = h->tick + 1;
    h->hist = std::move(fresh);
    return SIXDOF_OK;
} SIXDOF_ABI_CATCH(err_of(h))

// Ring and row width of a recorded component: the four recorded Body columns and the non-window component columns of the
// installed program — what sixdof_history_read accepts and sixdof_set_watch watches.  *ring_base is null while no ring is enabled.
static bool watch_lookup(const sixdof_handle* h, uint64_t id, const void** ring_base, size_t* w) {
    for (auto& b : h->body)
        if (id == b.id && b.ring >= 0) {
            *ring_base = h->hist.ring ? h->hist.body[b.ring].get() : nullptr;
            *w = b.width;
            return true;
        }
    for (size_t m = 0; m < h->custom_model.size(); m++) {
        if (h->custom_model[m] != id) continue;
        const Column* c = recorded_model_column(h, m);
        if (!c) return false;
        *ring_base = h->hist.ring && m < h->hist.model.size() ? h->hist.model[m].get() : nullptr;
        *w = static_cast<size_t>(c->width);
        return true;
    }
    return false;
}

int sixdof_history_read(sixdof_handle* h, uint64_t component_id, uint64_t tick, void* host_dst) try {
    if (!h || !host_dst) return SIXDOF_ERR_INVALID_ARGUMENT;
    const History& hs = h->hist;
    if (!hs.ring) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, "history_read: no history ring (sixdof_set_history)");
    const void* ring_base = nullptr;
    size_t w = 0;
    if (!watch_lookup(h, component_id, &ring_base, &w) || !ring_base)
        return h->fail(SIXDOF_ERR_COMPONENT_NOT_FOUND, "history_read: only world_pos / world_vel / world_accel / force and the component columns of a generated program are recorded");
    if (!sampled_range_ok(tick, 1, 1, hs.first_tick, h->tick, hs.ring))
        return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, "history_read: tick is not in the ring");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t block = static_cast<size_t>(h->desc.n_entities) * w * h->elem_size();
    const size_t slot = static_cast<size_t>(history_slot(tick, hs.ring));
    if (block) {
        HIP_TRY(h, h->copy.settle(host_dst, block));   // a lock an asynchronous read left over a part of the buffer
        HIP_TRY(h, hipMemcpyAsync(host_dst, static_cast<const char*>(ring_base) + slot * block, block, hipMemcpyDeviceToHost, h->stream.get()));
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream.get()));
    return SIXDOF_OK;
} SIXDOF_ABI_CATCH(err_of(h))

int sixdof_history_stream(sixdof_handle* h, uint64_t first_tick, uint64_t n_ticks, void* const host_dst[4]) try {
    if (!h || !host_dst) return SIXDOF_ERR_INVALID_ARGUMENT;
    const History& hs = h->hist;
    if (!hs.ring) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, "history_stream: no history ring (sixdof_set_history)");
    if (n_ticks == 0) return SIXDOF_OK;
    if (!sampled_range_ok(first_tick, n_ticks, 1, hs.first_tick, h->tick, hs.ring))
        return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, "history_stream: ticks are not (all) in the ring");
    HIP_TRY(h, hipSetDevice(h->device));
    CopyLane& lane = h->copy;
    HIP_TRY(h, lane.begin(h->stream.get()));            // everything recorded so far is in the ring after this
    const size_t n = h->desc.n_entities, es = h->elem_size();
    for (int k = 0; k < 4; k++) {
        if (!host_dst[k]) continue;
        const size_t block = n * h->body[k].width * es;
        if (!block) continue;
        // the run is contiguous in the ring except where it wraps: at most two copies per column
        const size_t slot0 = static_cast<size_t>(history_slot(first_tick, hs.ring));
        const size_t head = std::min<size_t>(n_ticks, hs.ring - slot0);
        char* dst = static_cast<char*>(host_dst[k]);
        const char* ring = hs.body[k].get<char>();
        HIP_TRY(h, lane.copy(dst, ring + slot0 * block, head * block, n_ticks * block));
        if (head < n_ticks) HIP_TRY(h, lane.copy(dst + head * block, ring, (n_ticks - head) * block, 0));
    }
    HIP_TRY(h, lane.end());
    // the one reader whose copies read the RING from the copy stream: sixdof_step holds back a batch that would overwrite these ticks,
    // and those of every earlier run that nothing has waited for yet (the hull of them all: a step held back needlessly is only late)
    const bool earlier = lane.stream_hi >= lane.stream_lo;
    lane.stream_lo = earlier ? std::min(lane.stream_lo, first_tick) : first_tick;
    lane.stream_hi = earlier ? std::max(lane.stream_hi, first_tick + n_ticks - 1) : first_tick + n_ticks - 1;
    return SIXDOF_OK;
} SIXDOF_ABI_CATCH(err_of(h))

int sixdof_set_watch(sixdof_handle* h, const uint64_t* component_ids, size_t n_components, const uint64_t* entity_ids,
                     size_t n_entities) try {
    if (!h || (!component_ids && n_components) || (!entity_ids && n_entities)) return SIXDOF_ERR_INVALID_ARGUMENT;
    if ((n_components == 0) != (n_entities == 0))
        return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, "set_watch: components without entities (or the reverse); 0 / 0 clears the watch");
    if (!h->bound) return h->fail(SIXDOF_ERR_COMPONENT_NOT_FOUND, "set_watch: bind Body columns first");
    HIP_TRY(h, hipSetDevice(h->device));
    // everything that can fail comes first: the previous watch stays as it is until the new one is complete
    for (size_t k = 0; k < n_components; k++) {
        const void* ring_base = nullptr;
        size_t w = 0;
        if (!watch_lookup(h, component_ids[k], &ring_base, &w))
            return h->fail(SIXDOF_ERR_COMPONENT_NOT_FOUND, "set_watch: only world_pos / world_vel / world_accel / force and the non-window component columns of a generated program are recorded");
    }
    std::vector<uint32_t> rows;
    if (const size_t bad = resolve_rows(row_map(h->joined_ids), entity_ids, n_entities, &rows); bad != n_entities)
        return h->fail(SIXDOF_ERR_ENTITY_MISMATCH, "set_watch: entity " + std::to_string(entity_ids[bad]) + " is not in the joined Body entity set");
    std::vector<uint64_t> ids(component_ids, component_ids + n_components);
    DeviceBuffer d_rows;
    if (n_entities) {
        HIP_TRY(h, d_rows.alloc(n_entities * sizeof(uint32_t)));
        HIP_TRY(h, hipMemcpy(d_rows.get(), rows.data(), n_entities * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream.get()));   // a gather in flight reads the old table
    h->drop_watch();
    h->watch_ids.swap(ids);
    h->d_watch_rows = std::move(d_rows);
    h->watch_m = n_entities;
    return SIXDOF_OK;
} SIXDOF_ABI_CATCH(err_of(h))

// A read whose results are computed on the compute stream, out of the ring into a device staging buffer, and brought from
// there to the caller's buffers, blocking or over the copy lane.  Its users: sixdof_watch_read, ring_bin_read (the envelopes and
// the quantiles) and time_scan_read (the extremes and the events).  The lane and the rules of the staging buffer live here and
// nowhere in the callers: add() the components, claim() the buffers, launch into them, deliver().
struct StagedRead {
    // one component: ring base and width as they are NOW, its block in the staging buffer (256-byte aligned), where it goes
    struct Part { const void* ring; size_t w, bytes, offset; void* host; };
    sixdof_handle* h;
    const char* who;        // the entry point, for its messages
    DeviceBuffer* stage;    // lives with whatever the entry point chose (the handle, the ring)
    std::vector<Part> parts;
    size_t stage_bytes = 0;

    // `per_width` elements of `elem` bytes for every element of a row; `unrecorded`: the message when the ring does not hold `id`
    // (host_needed = false: a read that delivers nothing, a scan that holds)
    int add(uint64_t id, void* host, size_t per_width, size_t elem, const char* unrecorded, bool host_needed = true) {
        Part p{};
        if (!watch_lookup(h, id, &p.ring, &p.w) || !p.ring) return h->fail(SIXDOF_ERR_COMPONENT_NOT_FOUND, std::string(who) + ": " + unrecorded);
        if (!host && host_needed) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, std::string(who) + ": null host buffer");
        p.host = host, p.bytes = per_width * p.w * elem, p.offset = stage_bytes;
        stage_bytes += (p.bytes + 255) / 256 * 256;
        parts.push_back(p);
        return SIXDOF_OK;
    }
    // a block of the staging buffer that belongs to no component (sixdof_history_events: the event planes)
    void add_block(void* host, size_t bytes) {
        parts.push_back(Part{nullptr, 1, bytes, stage_bytes, host});
        stage_bytes += (bytes + 255) / 256 * 256;
    }
    // After this the compute stream may write the staging buffer, large enough for every part, and `scratch` (if any) of at
    // least scratch_bytes.  A buffer that could not be grown is left empty: the next read allocates it again.
    int claim(DeviceBuffer* scratch = nullptr, size_t scratch_bytes = 0) {
        CopyLane& lane = h->copy;
        const bool grow_stage = stage_bytes > stage->bytes(), grow_scratch = scratch && scratch_bytes > scratch->bytes();
        if (grow_stage || grow_scratch) {
            // the copy stream may still read the old staging buffer (a previous asynchronous read), the compute stream may still use both
            if (lane.pending) HIP_TRY(h, hipStreamSynchronize(lane.stream.get()));
            HIP_TRY(h, hipStreamSynchronize(h->stream.get()));
            if (grow_stage) HIP_TRY(h, stage->alloc(stage_bytes));   // free first; on failure empty
            if (grow_scratch) HIP_TRY(h, scratch->alloc(scratch_bytes));
        }
        HIP_TRY(h, lane.hold(h->stream.get()));   // one staging buffer: the launches that follow overwrite it
        return SIXDOF_OK;
    }
    // The parts, complete in the staging buffer once the compute stream gets here, to the caller's buffers.
    int deliver(bool async) {
        CopyLane& lane = h->copy;
        const char* staged = stage->get<char>();
        if (!async) {
            for (const Part& p : parts)
                if (p.bytes) {
                    HIP_TRY(h, lane.settle(p.host, p.bytes));   // a lock an asynchronous read left over a part of the buffer
                    HIP_TRY(h, hipMemcpyAsync(p.host, staged + p.offset, p.bytes, hipMemcpyDeviceToHost, h->stream.get()));
                }
            HIP_TRY(h, hipStreamSynchronize(h->stream.get()));
            return SIXDOF_OK;
        }
        HIP_TRY(h, lane.begin(h->stream.get()));
        for (const Part& p : parts)
            if (p.bytes) HIP_TRY(h, lane.copy(p.host, staged + p.offset, p.bytes, p.bytes));
        HIP_TRY(h, lane.end());
        return SIXDOF_OK;
    }
};

// Ordering of the gather after the batch that recorded the ticks it reads.  With a ring enabled a handle neither replays
// hipGraphs nor submits AQL chains (graph_eligible needs !hist_ring): every recording launch — the step kernel, the pair
// and model kernels and their snapshot_tick_to_ring copies — is an eager launch on h->stream.get(), so the gather, launched on
// h->stream.get(), follows the batch's last launch by stream order, asynchronous steps included.  Were a ring ever recorded
// through the other two paths: hipGraphLaunch replays on h->stream.get() too (stream order again), and an AQL chain is waited
// for on the host before sixdof_step returns (aql::run_chain spins on its last packet), i.e. before this call can start.
// The ring is read on the compute stream only; the copy stream reads the staging buffer.  So the next batch, also on
// the compute stream, may overwrite the slots with no further wait, and stream_lo / stream_hi — the overwrite protection
// of a sixdof_history_stream copy that reads the RING from the copy stream — stay as that call left them.
int sixdof_watch_read(sixdof_handle* h, uint64_t first_tick, uint64_t n_samples, uint64_t every, void* const host_dst[],
                      uint32_t flags) try {
    if (!h) return SIXDOF_ERR_INVALID_ARGUMENT;
    if (flags & ~SIXDOF_WATCH_ASYNC) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, "watch_read: unknown flags");
    if (h->watch_ids.empty()) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, "watch_read: no watch (sixdof_set_watch)");
    if (!h->hist.ring) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, "watch_read: no history ring (sixdof_set_history)");
    if (every == 0) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, "watch_read: every must be at least 1");
    if (n_samples == 0) return SIXDOF_OK;
    if (!host_dst) return SIXDOF_ERR_INVALID_ARGUMENT;
    if (!sampled_range_ok(first_tick, n_samples, every, h->hist.first_tick, h->tick, h->hist.ring))
        return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, "watch_read: ticks are not (all) in the ring");
    const size_t n_comp = h->watch_ids.size(), es = h->elem_size(), m = h->watch_m;
    StagedRead rd{h, "watch_read", &h->d_watch_stage};
    for (size_t k = 0; k < n_comp; k++) {
        const int rc = rd.add(h->watch_ids[k], host_dst[k], m * static_cast<size_t>(n_samples), es,
                              "a watched component is no longer recorded (the program was replaced)");
        if (rc != SIXDOF_OK) return rc;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = rd.claim(); rc != SIXDOF_OK) return rc;
    for (size_t k0 = 0; k0 < n_comp; k0 += kHistoryGatherMax) {
        const uint32_t cnt = static_cast<uint32_t>(std::min<size_t>(kHistoryGatherMax, n_comp - k0));
        HistoryGatherArgs a{};
        for (uint32_t k = 0; k < cnt; k++) {
            a.c[k].ring = rd.parts[k0 + k].ring;
            a.c[k].out_offset = rd.parts[k0 + k].offset / es;
            a.c[k].w = static_cast<uint32_t>(rd.parts[k0 + k].w);
        }
        hipError_t e = launch_history_gather(a, cnt, h->d_watch_stage.get(), h->d_watch_rows.get<uint32_t>(), m, h->desc.n_entities, first_tick, n_samples,
                                             every, h->hist.ring, es, h->stream.get());
        if (e != hipSuccess) return h->hip_fail(e, "history_gather");
    }
    return rd.deliver((flags & SIXDOF_WATCH_ASYNC) != 0);
} SIXDOF_ABI_CATCH(err_of(h))

}  // extern "C"

// A per-tick reduction of ring components into (group, element) bins: sixdof_history_envelope and sixdof_history_quantiles.
// Ordering, ring reads and the copy lane exactly as for sixdof_watch_read above — the reduction's launches go on the compute
// stream behind the batch that recorded the ticks, only the staging buffer is read from the copy stream.  Stateless: components
// and widths are looked up per call.  What a reduction is:
struct RingBinSpec {
    const char* who;          // the entry point, for its messages
    uint32_t async_flag;      // the one flag it knows
    size_t planes;            // doubles per bin in the output
    size_t unit_bytes;        // scratch bytes per unit and sample
    const char* bins_limit;   // how its message ends when period x width exceeds kEnvelopeMaxBins
    bool rows_in_32_bits;     // its kernels count the rows of a group in 32 bits
    DeviceBuffer *stage, *scratch;
};
// Refuses, plans, launches and delivers.  own_checks() -> status: the entry point's own argument checks, in their place after
// the common four.  units(n, w, period): scratch units of one component and sample.  launch(args, count, stride, chunk, sample0,
// n_samples) -> hipError_t: one batch of at most kRingBinMaxComponents components x one chunk of samples; `stride` units of
// scratch per sample, `chunk` samples per launch (the last may be shorter) as the scratch buffer was sized.
template <class Checks, class Units, class Launch>
static int ring_bin_read(sixdof_handle* h, const RingBinSpec& spec, const uint64_t* component_ids, size_t n_components, uint64_t first_tick,
                         uint64_t n_samples, uint64_t every, uint32_t period, double* const host_dst[], uint32_t flags, Checks own_checks,
                         Units units, Launch launch) {
    const std::string who = spec.who;
    if (flags & ~spec.async_flag) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, who + ": unknown flags");
    if (!h->hist.ring) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, who + ": no history ring (sixdof_set_history)");
    if (every == 0) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, who + ": every must be at least 1");
    if (period == 0) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, who + ": period must be at least 1");
    if (int rc = own_checks(); rc != SIXDOF_OK) return rc;
    const uint64_t n = h->desc.n_entities;
    if (n % period != 0)
        return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, who + ": the " + std::to_string(n) + " rows are no multiple of period " + std::to_string(period));
    if (spec.rows_in_32_bits && (n / period) >> 32) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, who + ": more than 2^32 rows in a group");
    if (n_samples == 0 || n_components == 0) return SIXDOF_OK;
    if (!component_ids || !host_dst) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, who + ": null argument");
    if (!sampled_range_ok(first_tick, n_samples, every, h->hist.first_tick, h->tick, h->hist.ring))
        return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, who + ": ticks are not (all) in the ring");
    StagedRead rd{h, spec.who, spec.stage};
    std::vector<size_t> scratch_offset(n_components);   // per component: its units in a sample's scratch
    size_t stride = 0, launch_units = 0;
    for (size_t k = 0; k < n_components; k++) {
        const int rc = rd.add(component_ids[k], host_dst[k], static_cast<size_t>(n_samples) * period * spec.planes, sizeof(double),
                              "only world_pos / world_vel / world_accel / force and the non-window component columns of a generated program are recorded");
        if (rc != SIXDOF_OK) return rc;
        const size_t w = rd.parts[k].w;
        if (!envelope_supported(w, period))
            return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, who + ": period " + std::to_string(period) + " x width " + std::to_string(w) + " exceeds the " +
                                                            std::to_string(kEnvelopeMaxBins) + " (group, element) bins " + spec.bins_limit);
        if (k % kRingBinMaxComponents == 0) launch_units = 0;   // every launch of at most 32 components reuses the scratch
        scratch_offset[k] = launch_units;
        launch_units += units(n, static_cast<uint32_t>(w), period);
        stride = std::max(stride, launch_units);
    }
    if (n == 0) {      // nothing to reduce: count 0, the other planes NaN
        for (size_t k = 0; k < n_components; k++)
            for (size_t i = 0; i < rd.parts[k].bytes / sizeof(double); i++) host_dst[k][i] = i / rd.parts[k].w % spec.planes == 0 ? 0.0 : std::nan("");
        return SIXDOF_OK;
    }
    // samples per launch: the scratch of one launch stays within a fixed budget, and the grid's y extent below 2^16
    constexpr size_t kScratchBudget = size_t(64) << 20;
    const size_t per_sample = stride * spec.unit_bytes;
    const uint64_t chunk = std::min<uint64_t>({n_samples, 65535, std::max<size_t>(1, kScratchBudget / per_sample)});
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = rd.claim(spec.scratch, chunk * per_sample); rc != SIXDOF_OK) return rc;
    for (size_t k0 = 0; k0 < n_components; k0 += kRingBinMaxComponents) {
        const uint32_t cnt = static_cast<uint32_t>(std::min<size_t>(kRingBinMaxComponents, n_components - k0));
        RingBinArgs a{};
        for (uint32_t k = 0; k < cnt; k++) {
            a.c[k].ring = rd.parts[k0 + k].ring;
            a.c[k].out_offset = rd.parts[k0 + k].offset / sizeof(double);
            a.c[k].scratch_offset = scratch_offset[k0 + k];
            a.c[k].w = static_cast<uint32_t>(rd.parts[k0 + k].w);
        }
        for (uint64_t s0 = 0; s0 < n_samples; s0 += chunk) {
            hipError_t e = launch(a, cnt, stride, chunk, s0, std::min<uint64_t>(chunk, n_samples - s0));
            if (e != hipSuccess) return h->hip_fail(e, spec.who);
        }
    }
    return rd.deliver((flags & spec.async_flag) != 0);
}

extern "C" {

// The envelopes of sampled ticks: two reduction launches per batch and chunk, a scratch unit is one partial record.
int sixdof_history_envelope(sixdof_handle* h, const uint64_t* component_ids, size_t n_components, uint64_t first_tick,
                            uint64_t n_samples, uint64_t every, uint32_t period, double* const host_dst[], uint32_t flags) try {
    if (!h) return SIXDOF_ERR_INVALID_ARGUMENT;
    History& hs = h->hist;
    const RingBinSpec spec{"history_envelope", SIXDOF_ENVELOPE_ASYNC, kEnvelopeStats, sizeof(EnvelopePartial), "one block keeps apart", false,
                           &hs.env_stage, &hs.env_partial};
    return ring_bin_read(
        h, spec, component_ids, n_components, first_tick, n_samples, every, period, host_dst, flags, [] { return int(SIXDOF_OK); },
        [](uint64_t n, uint32_t w, uint32_t p) {
            const EnvelopeGeom g = envelope_geom(n, w, p);
            return static_cast<size_t>(g.blocks) * g.bins;
        },
        [&](const RingBinArgs& a, uint32_t cnt, size_t stride, uint64_t, uint64_t s0, uint64_t ns) {
            return launch_history_envelope(a, cnt, hs.env_stage.get<double>(), hs.env_partial.get(), stride, h->desc.n_entities, period, first_tick, s0, ns,
                                           every, hs.ring, h->elem_size(), h->stream.get());
        });
} SIXDOF_ABI_CATCH(err_of(h))

// Exact order statistics of sampled ticks: the passes of a radix select per batch and chunk, a scratch unit is one (bin, rank)
// slot — its histogram and, behind the histograms of a whole chunk, its state.
int sixdof_history_quantiles(sixdof_handle* h, const uint64_t* component_ids, size_t n_components, uint64_t first_tick,
                             uint64_t n_samples, uint64_t every, uint32_t period, const uint32_t* rank_num, uint32_t rank_den,
                             size_t n_ranks, double* const host_dst[], uint32_t flags) try {
    if (!h) return SIXDOF_ERR_INVALID_ARGUMENT;
    History& hs = h->hist;
    QuantileRanks ranks{};
    auto rank_checks = [&] {
        if (n_ranks == 0 || n_ranks > SIXDOF_QUANTILE_MAX_RANKS)
            return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, "history_quantiles: " + std::to_string(n_ranks) + " ranks, 1 to " + std::to_string(SIXDOF_QUANTILE_MAX_RANKS) + " can be asked for");
        if (!rank_num) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, "history_quantiles: null ranks");
        if (rank_den == 0) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, "history_quantiles: the ranks' denominator must be at least 1");
        ranks.den = rank_den, ranks.count = static_cast<uint32_t>(n_ranks);
        for (size_t i = 0; i < n_ranks; i++) {
            if (rank_num[i] > rank_den)
                return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, "history_quantiles: rank " + std::to_string(rank_num[i]) + " / " + std::to_string(rank_den) + " is above 1");
            ranks.num[i] = rank_num[i];
        }
        return int(SIXDOF_OK);
    };
    constexpr size_t kHistBytes = kQuantileDigits * sizeof(uint32_t);
    const RingBinSpec spec{"history_quantiles", SIXDOF_QUANTILE_ASYNC, 1 + 2 * n_ranks, kHistBytes + sizeof(QuantileSlot), "of one read", true,
                           &hs.quant_stage, &hs.quant_scratch};
    return ring_bin_read(
        h, spec, component_ids, n_components, first_tick, n_samples, every, period, host_dst, flags, rank_checks,
        [&](uint64_t, uint32_t w, uint32_t p) { return static_cast<size_t>(p) * w * n_ranks; },
        [&](const RingBinArgs& a, uint32_t cnt, size_t stride, uint64_t chunk, uint64_t s0, uint64_t ns) {
            char* scratch = hs.quant_scratch.get<char>();
            return launch_history_quantiles(a, cnt, ranks, hs.quant_stage.get<double>(), scratch, scratch + chunk * stride * kHistBytes, stride,
                                            h->desc.n_entities, period, first_tick, s0, ns, every, hs.ring, h->elem_size(), h->stream.get());
        });
} SIXDOF_ABI_CATCH(err_of(h))

// The joint moments of sampled ticks: count, mean vector and co-moment matrix of 2 .. 6 channels, two reduction launches per chunk
// of samples.  Ordering, ring reads and the copy lane exactly as for sixdof_history_envelope; not through ring_bin_read, whose
// contract — bins, output blocks, scratch units — is per component: here a ROW is the unit, its channels may come from several
// components and there is one output block.  Stateless: the channels are looked up per call.
int sixdof_history_covariance(sixdof_handle* h, const sixdof_cov_channel* channels, size_t n_channels, uint64_t first_tick, uint64_t n_samples,
                              uint64_t every, uint32_t period, double* host_dst, uint32_t flags) try {
    if (!h) return SIXDOF_ERR_INVALID_ARGUMENT;
    History& hs = h->hist;
    const std::string who = "history_covariance";
    if (flags & ~SIXDOF_COVARIANCE_ASYNC) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, who + ": unknown flags");
    if (!hs.ring) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, who + ": no history ring (sixdof_set_history)");
    if (every == 0) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, who + ": every must be at least 1");
    if (period == 0) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, who + ": period must be at least 1");
    if (n_channels == 1)
        return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, who + ": one channel has no co-moments: its count, mean and m2 are sixdof_history_envelope's");
    if (n_channels < 2 || n_channels > SIXDOF_COVARIANCE_MAX_CHANNELS)
        return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, who + ": " + std::to_string(n_channels) + " channels, 2 to " + std::to_string(SIXDOF_COVARIANCE_MAX_CHANNELS) + " can be asked for");
    const uint64_t n = h->desc.n_entities;
    if (n % period != 0)
        return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, who + ": the " + std::to_string(n) + " rows are no multiple of period " + std::to_string(period));
    if (period > kCovarianceMaxPeriod)
        return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, who + ": period " + std::to_string(period) + " exceeds the " + std::to_string(kCovarianceMaxPeriod) + " groups one block keeps apart");
    if (n_samples == 0) return SIXDOF_OK;
    if (!channels || !host_dst) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, who + ": null argument");
    const uint32_t k = static_cast<uint32_t>(n_channels);
    const size_t fields = covariance_fields(k);
    StagedRead rd{h, "history_covariance", &hs.cov_stage};
    CovarianceArgs args{};
    std::vector<uint64_t> seen;   // a component is looked up once, however many channels name it
    for (uint32_t c = 0; c < k; c++) {
        if (channels[c].reserved != 0) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, who + ": channel " + std::to_string(c) + ": reserved must be 0");
        size_t at = std::find(seen.begin(), seen.end(), channels[c].component_id) - seen.begin();
        if (at == seen.size()) {
            const int rc = rd.add(channels[c].component_id, nullptr, 0, sizeof(double),
                                  "only world_pos / world_vel / world_accel / force and the non-window component columns of a generated program are recorded", false);
            if (rc != SIXDOF_OK) return rc;
            seen.push_back(channels[c].component_id);
        }
        const StagedRead::Part& p = rd.parts[at];
        if (channels[c].element >= p.w)
            return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, who + ": channel " + std::to_string(c) + ": element " + std::to_string(channels[c].element) + " of a component " +
                                                            std::to_string(p.w) + " wide");
        args.c[c] = CovarianceChannel{p.ring, static_cast<uint32_t>(p.w), channels[c].element};
    }
    if (!sampled_range_ok(first_tick, n_samples, every, hs.first_tick, h->tick, hs.ring))
        return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, who + ": ticks are not (all) in the ring");
    const size_t out_doubles = static_cast<size_t>(n_samples) * period * fields;
    if (n == 0) {   // nothing to reduce: count 0, everything else NaN
        for (size_t i = 0; i < out_doubles; i++) host_dst[i] = i % fields == 0 ? 0.0 : std::nan("");
        return SIXDOF_OK;
    }
    rd.add_block(host_dst, out_doubles * sizeof(double));
    // samples per launch: the scratch of one launch stays within a fixed budget, and the grid's y extent below 2^16
    constexpr size_t kScratchBudget = size_t(64) << 20;
    const size_t stride = covariance_scratch_doubles(covariance_geom(n, period), k, period), per_sample = stride * sizeof(double);
    const char* chunk_env = std::getenv("SIXDOF_COVARIANCE_CHUNK");   // samples per launch, at most the plan's choice (tests)
    const uint64_t forced = chunk_env ? std::strtoull(chunk_env, nullptr, 10) : 0;
    uint64_t chunk = std::min<uint64_t>({n_samples, 65535, std::max<size_t>(1, kScratchBudget / per_sample)});
    if (forced) chunk = std::min(chunk, forced);
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = rd.claim(&hs.cov_partial, chunk * per_sample); rc != SIXDOF_OK) return rc;
    double* staged = reinterpret_cast<double*>(hs.cov_stage.get<char>() + rd.parts.back().offset);
    for (uint64_t s0 = 0; s0 < n_samples; s0 += chunk) {
        hipError_t e = launch_history_covariance(args, k, staged, hs.cov_partial.get(), stride, n, period, first_tick, s0, std::min<uint64_t>(chunk, n_samples - s0), every,
                                                 hs.ring, h->elem_size(), h->stream.get());
        if (e != hipSuccess) return h->hip_fail(e, "history_covariance");
    }
    return rd.deliver((flags & SIXDOF_COVARIANCE_ASYNC) != 0);
} SIXDOF_ABI_CATCH(err_of(h))

}  // extern "C"

// A scan of the ring over time: sixdof_history_extremes, sixdof_history_events, sixdof_history_norms, sixdof_history_norm_events and sixdof_history_dwell.  Ordering, ring reads and the copy lane exactly
// as for sixdof_watch_read above; not through ring_bin_read, whose output and chunk rule are per sample: here ALL samples of the
// range go into one launch, cut into time segments (time_scan.hpp), and the output is per row or run.  The staging buffer is the
// accumulator: a call with `continues` merges into what the previous call left there, a call with `holds` delivers nothing.
// Commit on success: the accumulator is invalid from the first step that can fail in the runtime to the last enqueue.  What a
// scan is:
struct TimeScanSpec {
    const char* who;                                             // the entry point, for its messages
    uint32_t async, continues, holds;                            // the three flags it knows
    const char* continue_name;                                   // how `continues` is spelled in its messages
    const char* accumulator_of;                                  // what a continuing call has to repeat, for its message
    const char* segments_env;                                    // 0 or unset: the plan's choice (A/B runs, tests)
    uint32_t (*segments)(uint64_t units, uint64_t n_samples);    // the plan's choice
    uint32_t fields;                                             // 64-bit words of a record in scratch
    History::TimeScan* scan;
};
// Refuses, plans, launches, delivers and commits.  own_checks(nothing) -> status: the entry point's own argument checks, in their
// place after the common three; `nothing` arrives as "no samples" and may be set where there is nothing to read for another
// reason, the call then returns SIXDOF_OK.  parts(rd, next, units) -> status: adds the StagedRead parts, fills next.signature, .rings
// and .widths, and appends the units of every launch.  launch(rd, i, units, segments, merge_into) -> status: launch i, its segment
// records within a fixed scratch budget.
template <class Checks, class Parts, class Launch>
static int time_scan_read(sixdof_handle* h, const TimeScanSpec& spec, uint64_t first_tick, uint64_t n_samples, uint64_t every, uint32_t flags,
                          Checks own_checks, Parts parts, Launch launch) {
    const std::string who = spec.who;
    if (flags & ~(spec.async | spec.continues | spec.holds)) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, who + ": unknown flags");
    History& hs = h->hist;
    if (!hs.ring) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, who + ": no history ring (sixdof_set_history)");
    if (every == 0) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, who + ": every must be at least 1");
    bool nothing = n_samples == 0;
    if (int rc = own_checks(nothing); rc != SIXDOF_OK) return rc;
    if (nothing) return SIXDOF_OK;
    if (!sampled_range_ok(first_tick, n_samples, every, hs.first_tick, h->tick, hs.ring))
        return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, who + ": ticks are not (all) in the ring");
    if (!scan_ticks_ok(first_tick, n_samples, every))
        return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, who + ": a sampled tick of 2^53 or more has no double of its own");
    StagedRead rd{h, spec.who, &spec.scan->stage};
    History::ScanState next;
    next.n = h->desc.n_entities, next.last_tick = first_tick + (n_samples - 1) * every;
    std::vector<uint64_t> units;
    if (int rc = parts(rd, next, units); rc != SIXDOF_OK) return rc;
    History::ScanState& acc = spec.scan->acc;
    const bool merge_into = (flags & spec.continues) != 0;
    if (merge_into) {
        const std::string what = who + ": " + spec.continue_name + ": ";
        if (!acc.valid || acc.n != next.n || acc.signature != next.signature || acc.rings != next.rings || acc.widths != next.widths)
            return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, what + "there is no accumulator of these " + spec.accumulator_of + " to continue "
                                                               "(the previous call failed or read something else, or the ring, the columns or the program were replaced since)");
        if (first_tick <= acc.last_tick)
            return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, what + "first_tick " + std::to_string(first_tick) + " is not above tick " + std::to_string(acc.last_tick) +
                                                               ", the last one accumulated");
    }
    const char* forced_env = std::getenv(spec.segments_env);
    const uint64_t forced = forced_env ? std::strtoull(forced_env, nullptr, 10) : 0;
    constexpr uint64_t kScratchBudget = uint64_t(64) << 20;
    std::vector<uint32_t> segments;
    uint64_t scratch_bytes = 0;
    for (uint64_t u : units) {
        const uint32_t s = forced ? scan_clamp_segments(forced, n_samples) : spec.segments(u, n_samples);
        segments.push_back(scan_fit_segments(s, u, spec.fields, kScratchBudget));
        scratch_bytes = std::max(scratch_bytes, scan_scratch_bytes(segments.back(), u, spec.fields));
    }
    HIP_TRY(h, hipSetDevice(h->device));
    acc.valid = false;
    if (int rc = rd.claim(&spec.scan->scratch, static_cast<size_t>(scratch_bytes)); rc != SIXDOF_OK) return rc;
    for (size_t i = 0; i < units.size(); i++)
        if (int rc = launch(rd, i, units[i], segments[i], merge_into); rc != SIXDOF_OK) return rc;
    if (!(flags & spec.holds))
        if (int rc = rd.deliver((flags & spec.async) != 0); rc != SIXDOF_OK) return rc;
    acc = std::move(next);
    acc.valid = true;
    return SIXDOF_OK;
}

static const char* const kOnlyRecorded = "only world_pos / world_vel / world_accel / force and the non-window component columns of a generated program are recorded";

// One probe of sixdof_history_norms, sixdof_history_norm_events or sixdof_history_dwell, checked against the ring and resolved into what the kernels
// see; `which` names it in the messages.
static int norm_probe_resolve(sixdof_handle* h, const std::string& which, const sixdof_norm_probe& p, uint32_t period, NormsProbe& d) {
    if (p.flags & ~SIXDOF_NORM_MINUS) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, which + ": unknown flags " + std::to_string(p.flags));
    if (p.count == 0 || p.count > SIXDOF_NORM_MAX_COUNT)
        return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, which + ": count " + std::to_string(p.count) + ", 1 to " + std::to_string(SIXDOF_NORM_MAX_COUNT) + " elements can be asked for");
    const bool minus = (p.flags & SIXDOF_NORM_MINUS) != 0;
    d.count = p.count, d.flags = p.flags;
    for (int side = 0; side < (minus ? 2 : 1); side++) {
        const char* name = side ? " (minus)" : "";
        const uint32_t element = side ? p.minus_element : p.element, group = side ? p.minus_group : p.group;
        if (group >= period)
            return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, which + name + ": group " + std::to_string(group) + " is not below period " + std::to_string(period));
        const void* ring = nullptr;
        size_t w = 0;
        if (!watch_lookup(h, side ? p.minus_component_id : p.component_id, &ring, &w) || !ring)
            return h->fail(SIXDOF_ERR_COMPONENT_NOT_FOUND, which + name + ": " + kOnlyRecorded);
        if (uint64_t(element) + p.count > w)
            return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, which + name + ": elements " + std::to_string(element) + " .. " + std::to_string(uint64_t(element) + p.count - 1) +
                                                            " are not all below the component's width " + std::to_string(w));
        if (side) d.ring_b = ring, d.w_b = static_cast<uint32_t>(w), d.element_b = element, d.group_b = group;
        else d.ring_a = ring, d.w_a = static_cast<uint32_t>(w), d.element_a = element, d.group_a = group;
    }
    return SIXDOF_OK;
}

// What a continuing call has to repeat of one probe: its eight words, and the ring and width of either side as resolved.
static void norm_probe_sign(const sixdof_norm_probe& p, const NormsProbe& d, History::ScanState& next) {
    next.signature.insert(next.signature.end(), {p.component_id, p.minus_component_id, p.element, p.minus_element, p.group, p.minus_group, p.count, p.flags});
    next.rings.push_back(d.ring_a), next.widths.push_back(d.w_a);
    if (p.flags & SIXDOF_NORM_MINUS) next.rings.push_back(d.ring_b), next.widths.push_back(d.w_b);
}

// The refusals of every scan per run (sixdof_history_events, sixdof_history_norms, sixdof_history_norm_events, sixdof_history_dwell), the first of its own
// checks: `count` of its `noun` outside 1 .. max, no period, rows that are no whole runs.
static int run_scan_checks(sixdof_handle* h, const std::string& who, size_t count, const char* noun, size_t max, uint32_t period) {
    const uint64_t n = h->desc.n_entities;
    if (count == 0 || count > max)
        return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, who + ": " + std::to_string(count) + " " + noun + ", 1 to " + std::to_string(max) + " can be asked for");
    if (period == 0) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, who + ": period must be at least 1");
    if (n % period != 0)
        return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, who + ": the " + std::to_string(n) + " rows are no multiple of period " + std::to_string(period));
    return SIXDOF_OK;
}

// The first event of every run per trigger, and the rows of the captured components at it: sixdof_history_events and
// sixdof_history_norm_events, which differ in the trigger alone.  One walk (and merge) launch covers all triggers, a unit is one
// (trigger, run); one capture launch behind it covers at most kRingBinMaxComponents captured components.  The accumulator is the
// record buffer (what the rule continues from) together with the staging buffer (the event planes, rewritten by every call, and the
// captures, of which a continuing call rewrites only the runs whose event it saw).  What an entry point supplies:
// resolve(k, which) -> status checks trigger k past its op and mode and fills the walk's arguments; sign(k, next) appends its
// signature words, rings and widths; walk(segments, merge_into) launches the walk; capture_args() are the triggers as
// launch_events_capture reads them, asked for once the walk is launched.
template <class Trigger, class Resolve, class Sign, class Walk, class CaptureArgs>
static int run_events_read(sixdof_handle* h, const TimeScanSpec& spec, size_t max_triggers, const Trigger* triggers, size_t n_triggers,
                           const uint64_t* capture_ids, size_t n_captures, uint32_t period, uint64_t first_tick, uint64_t n_samples, uint64_t every,
                           double* event_dst, double* const capture_dst[], uint32_t flags, Resolve resolve, Sign sign, Walk walk, CaptureArgs capture_args) {
    History& hs = h->hist;
    History::TimeScan& sc = *spec.scan;
    const std::string who = spec.who, capture_label = who + " capture";
    const bool hold = (flags & spec.holds) != 0;
    const uint64_t n = h->desc.n_entities;
    const uint32_t nt = static_cast<uint32_t>(n_triggers);
    return time_scan_read(
        h, spec, first_tick, n_samples, every, flags,
        [&](bool&) -> int {
            if (int rc = run_scan_checks(h, who, n_triggers, "triggers", max_triggers, period); rc != SIXDOF_OK) return rc;
            if (!triggers || (n_captures && !capture_ids) || (!hold && (!event_dst || (n_captures && !capture_dst))))
                return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, who + ": null argument");
            for (size_t k = 0; k < n_triggers; k++) {
                const Trigger& t = triggers[k];
                const std::string which = who + ": trigger " + std::to_string(k);
                if (t.op > SIXDOF_EVENT_GE) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, which + ": unknown op " + std::to_string(t.op));
                if (t.mode > SIXDOF_EVENT_CROSSING) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, which + ": unknown mode " + std::to_string(t.mode));
                if (int rc = resolve(k, which); rc != SIXDOF_OK) return rc;
            }
            return SIXDOF_OK;
        },
        [&](StagedRead& rd, History::ScanState& next, std::vector<uint64_t>& units) -> int {
            units.push_back(n / period * n_triggers);
            rd.add_block(hold ? nullptr : event_dst, static_cast<size_t>(units[0]) * kEventsPlanes * sizeof(double));
            next.signature = {n_triggers, period, n_captures};
            for (uint32_t k = 0; k < nt; k++) sign(k, next);
            for (size_t k = 0; k < n_captures; k++) {
                const int rc = rd.add(capture_ids[k], hold ? nullptr : capture_dst[k], static_cast<size_t>(n) * n_triggers, sizeof(double), kOnlyRecorded, !hold);
                if (rc != SIXDOF_OK) return rc;
                next.signature.push_back(capture_ids[k]);
                next.rings.push_back(rd.parts[1 + k].ring), next.widths.push_back(rd.parts[1 + k].w);
            }
            return SIXDOF_OK;
        },
        [&](const StagedRead& rd, size_t, uint64_t units, uint32_t segments, bool merge_into) -> int {
            if (events_record_bytes(units) > sc.rec.bytes()) {   // never for a continuing call: its records are as large as the accumulator's
                HIP_TRY(h, hipStreamSynchronize(h->stream.get()));   // an earlier call's launches may still use the old buffer
                HIP_TRY(h, sc.rec.alloc(static_cast<size_t>(events_record_bytes(units))));
            }
            hipError_t e = walk(segments, merge_into);
            if (e != hipSuccess) return h->hip_fail(e, spec.who);
            const EventsArgs modes = capture_args();
            for (size_t k0 = 0; k0 < n_captures; k0 += kRingBinMaxComponents) {
                const uint32_t cnt = static_cast<uint32_t>(std::min<size_t>(kRingBinMaxComponents, n_captures - k0));
                RingBinArgs c{};
                for (uint32_t k = 0; k < cnt; k++) {
                    const StagedRead::Part& p = rd.parts[1 + k0 + k];
                    c.c[k].ring = p.ring, c.c[k].out_offset = p.offset / sizeof(double), c.c[k].w = static_cast<uint32_t>(p.w);
                }
                e = launch_events_capture(modes, nt, c, cnt, sc.rec.get(), sc.stage.get<double>(), merge_into, n, period, first_tick, n_samples, every, hs.ring,
                                          h->elem_size(), h->stream.get());
                if (e != hipSuccess) return h->hip_fail(e, capture_label.c_str());
            }
            return SIXDOF_OK;
        });
}

extern "C" {

// The extremes of every row over the sampled ticks of a range: one walk (and merge) launch per batch of at most
// kRingBinMaxComponents components, a unit is one element of a row.
int sixdof_history_extremes(sixdof_handle* h, const uint64_t* component_ids, size_t n_components, uint64_t first_tick,
                            uint64_t n_samples, uint64_t every, double* const host_dst[], uint32_t flags) try {
    if (!h) return SIXDOF_ERR_INVALID_ARGUMENT;
    History& hs = h->hist;
    const TimeScanSpec spec{"history_extremes", SIXDOF_EXTREMES_ASYNC, SIXDOF_EXTREMES_CONTINUE, SIXDOF_EXTREMES_HOLD, "SIXDOF_EXTREMES_CONTINUE",
                            "components, rows and rings", "SIXDOF_EXTREMES_SEGMENTS", extremes_segments, kExtremesFields, &hs.extremes};
    const bool hold = (flags & SIXDOF_EXTREMES_HOLD) != 0;
    const uint64_t n = h->desc.n_entities;
    return time_scan_read(
        h, spec, first_tick, n_samples, every, flags,
        [&](bool& nothing) -> int {
            nothing = nothing || n_components == 0;
            if (nothing) return SIXDOF_OK;
            if (!component_ids || (!host_dst && !hold)) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, "history_extremes: null argument");
            return SIXDOF_OK;
        },
        [&](StagedRead& rd, History::ScanState& next, std::vector<uint64_t>& units) -> int {
            for (size_t k = 0; k < n_components; k++) {
                const int rc = rd.add(component_ids[k], hold ? nullptr : host_dst[k], static_cast<size_t>(n) * kExtremesPlanes, sizeof(double), kOnlyRecorded, !hold);
                if (rc != SIXDOF_OK) return rc;
                if (k % kRingBinMaxComponents == 0) units.push_back(0);
                units.back() += n * rd.parts[k].w;
                next.rings.push_back(rd.parts[k].ring), next.widths.push_back(rd.parts[k].w);
            }
            next.signature.assign(component_ids, component_ids + n_components);
            return SIXDOF_OK;
        },
        [&](const StagedRead& rd, size_t i, uint64_t units, uint32_t segments, bool merge_into) -> int {
            const size_t k0 = i * kRingBinMaxComponents;
            const uint32_t cnt = static_cast<uint32_t>(std::min<size_t>(kRingBinMaxComponents, n_components - k0));
            RingBinArgs a{};
            uint64_t unit0 = 0;
            for (uint32_t k = 0; k < cnt; k++) {
                const StagedRead::Part& p = rd.parts[k0 + k];
                a.c[k].ring = p.ring;
                a.c[k].out_offset = p.offset / sizeof(double);
                a.c[k].scratch_offset = unit0;
                a.c[k].w = static_cast<uint32_t>(p.w);
                unit0 += n * p.w;
            }
            hipError_t e = launch_history_extremes(a, cnt, hs.extremes.stage.get<double>(), hs.extremes.scratch.get(), units, segments, merge_into, n, first_tick,
                                                   n_samples, every, hs.ring, h->elem_size(), h->stream.get());
            return e == hipSuccess ? int(SIXDOF_OK) : h->hip_fail(e, "history_extremes");
        });
} SIXDOF_ABI_CATCH(err_of(h))

// run_events_read on one element of a row.
int sixdof_history_events(sixdof_handle* h, const sixdof_event_trigger* triggers, size_t n_triggers, const uint64_t* capture_ids,
                          size_t n_captures, uint32_t period, uint64_t first_tick, uint64_t n_samples, uint64_t every,
                          double* event_dst, double* const capture_dst[], uint32_t flags) try {
    if (!h) return SIXDOF_ERR_INVALID_ARGUMENT;
    History& hs = h->hist;
    History::TimeScan& sc = hs.events;
    const TimeScanSpec spec{"history_events", SIXDOF_EVENTS_ASYNC, SIXDOF_EVENTS_CONTINUE, SIXDOF_EVENTS_HOLD, "SIXDOF_EVENTS_CONTINUE",
                            "triggers, captures, period, rows and rings", "SIXDOF_EVENTS_SEGMENTS", events_segments, kEventsFields, &sc};
    EventsArgs a{};
    return run_events_read(
        h, spec, SIXDOF_EVENTS_MAX_TRIGGERS, triggers, n_triggers, capture_ids, n_captures, period, first_tick, n_samples, every, event_dst, capture_dst, flags,
        [&](size_t k, const std::string& which) -> int {
            const sixdof_event_trigger& t = triggers[k];
            if (!std::isfinite(t.level)) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, which + ": the level is not finite");
            if (t.group >= period) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, which + ": group " + std::to_string(t.group) + " is not below period " + std::to_string(period));
            size_t w = 0;
            if (!watch_lookup(h, t.component_id, &a.t[k].ring, &w) || !a.t[k].ring) return h->fail(SIXDOF_ERR_COMPONENT_NOT_FOUND, which + ": " + kOnlyRecorded);
            if (t.element >= w) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, which + ": element " + std::to_string(t.element) + " is not below the component's width " + std::to_string(w));
            a.t[k].level = t.level, a.t[k].w = static_cast<uint32_t>(w), a.t[k].element = t.element, a.t[k].group = t.group, a.t[k].op = t.op, a.t[k].mode = t.mode;
            return SIXDOF_OK;
        },
        [&](size_t k, History::ScanState& next) {
            const sixdof_event_trigger& t = triggers[k];
            uint64_t level;
            std::memcpy(&level, &t.level, sizeof(level));
            next.signature.insert(next.signature.end(), {t.component_id, t.element, t.group, t.op, t.mode, level});
            next.rings.push_back(a.t[k].ring), next.widths.push_back(a.t[k].w);
        },
        [&](uint32_t segments, bool merge_into) {
            return launch_history_events(a, static_cast<uint32_t>(n_triggers), sc.rec.get(), sc.stage.get<double>(), sc.scratch.get(), segments, merge_into,
                                         h->desc.n_entities, period, first_tick, n_samples, every, hs.ring, h->elem_size(), h->stream.get());
        },
        [&] { return a; });
} SIXDOF_ABI_CATCH(err_of(h))

// The extremes of a squared vector length or separation per probe and run.  One walk (and merge) launch covers all probes, a unit
// is one (probe, run); the accumulator is the staging buffer, as for the extremes.
int sixdof_history_norms(sixdof_handle* h, const sixdof_norm_probe* probes, size_t n_probes, uint32_t period, uint64_t first_tick, uint64_t n_samples,
                         uint64_t every, double* host_dst, uint32_t flags) try {
    if (!h) return SIXDOF_ERR_INVALID_ARGUMENT;
    History& hs = h->hist;
    History::TimeScan& sc = hs.norms;
    const TimeScanSpec spec{"history_norms", SIXDOF_NORMS_ASYNC, SIXDOF_NORMS_CONTINUE, SIXDOF_NORMS_HOLD, "SIXDOF_NORMS_CONTINUE",
                            "probes, period, rows and rings", "SIXDOF_NORMS_SEGMENTS", norms_segments, kNormsFields, &sc};
    const std::string who = spec.who;
    const bool hold = (flags & SIXDOF_NORMS_HOLD) != 0;
    const uint64_t n = h->desc.n_entities;
    const uint32_t np = static_cast<uint32_t>(n_probes);
    NormsArgs a{};
    return time_scan_read(
        h, spec, first_tick, n_samples, every, flags,
        [&](bool&) -> int {
            if (int rc = run_scan_checks(h, who, n_probes, "probes", SIXDOF_NORMS_MAX_PROBES, period); rc != SIXDOF_OK) return rc;
            if (!probes || (!hold && !host_dst)) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, who + ": null argument");
            for (size_t k = 0; k < n_probes; k++)
                if (int rc = norm_probe_resolve(h, who + ": probe " + std::to_string(k), probes[k], period, a.p[k]); rc != SIXDOF_OK) return rc;
            return SIXDOF_OK;
        },
        [&](StagedRead& rd, History::ScanState& next, std::vector<uint64_t>& units) -> int {
            units.push_back(n / period * n_probes);
            rd.add_block(hold ? nullptr : host_dst, static_cast<size_t>(units[0]) * kNormsPlanes * sizeof(double));
            next.signature = {n_probes, period};
            for (uint32_t k = 0; k < np; k++) norm_probe_sign(probes[k], a.p[k], next);
            return SIXDOF_OK;
        },
        [&](const StagedRead&, size_t, uint64_t, uint32_t segments, bool merge_into) -> int {
            hipError_t e = launch_history_norms(a, np, sc.stage.get<double>(), sc.scratch.get(), segments, merge_into, n, period, first_tick, n_samples, every, hs.ring,
                                                h->elem_size(), h->stream.get());
            return e == hipSuccess ? int(SIXDOF_OK) : h->hip_fail(e, "history_norms");
        });
} SIXDOF_ABI_CATCH(err_of(h))

// run_events_read on a squared vector length or separation: the probes of sixdof_history_norms, and the events' own capture launches
// handed the triggers' modes (norm_events_capture_args).
int sixdof_history_norm_events(sixdof_handle* h, const sixdof_norm_trigger* triggers, size_t n_triggers, const uint64_t* capture_ids,
                               size_t n_captures, uint32_t period, uint64_t first_tick, uint64_t n_samples, uint64_t every,
                               double* event_dst, double* const capture_dst[], uint32_t flags) try {
    if (!h) return SIXDOF_ERR_INVALID_ARGUMENT;
    History& hs = h->hist;
    History::TimeScan& sc = hs.norm_events;
    const TimeScanSpec spec{"history_norm_events", SIXDOF_NORM_EVENTS_ASYNC, SIXDOF_NORM_EVENTS_CONTINUE, SIXDOF_NORM_EVENTS_HOLD, "SIXDOF_NORM_EVENTS_CONTINUE",
                            "triggers, captures, period, rows and rings", "SIXDOF_NORM_EVENTS_SEGMENTS", norm_events_segments, kNormEventsFields, &sc};
    const uint32_t nt = static_cast<uint32_t>(n_triggers);
    NormEventsArgs a{};
    return run_events_read(
        h, spec, SIXDOF_NORM_EVENTS_MAX_TRIGGERS, triggers, n_triggers, capture_ids, n_captures, period, first_tick, n_samples, every, event_dst, capture_dst, flags,
        [&](size_t k, const std::string& which) -> int {
            const sixdof_norm_trigger& t = triggers[k];
            if (!std::isfinite(t.level_sq) || t.level_sq < 0.0) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, which + ": the squared level is not finite or is below 0");
            if (int rc = norm_probe_resolve(h, which, t.probe, period, a.t[k].probe); rc != SIXDOF_OK) return rc;
            a.t[k].level_sq = t.level_sq, a.t[k].op = t.op, a.t[k].mode = t.mode;
            return SIXDOF_OK;
        },
        [&](size_t k, History::ScanState& next) {
            const sixdof_norm_trigger& t = triggers[k];
            uint64_t level;
            std::memcpy(&level, &t.level_sq, sizeof(level));
            norm_probe_sign(t.probe, a.t[k].probe, next);
            next.signature.insert(next.signature.end(), {level, t.op, t.mode});
        },
        [&](uint32_t segments, bool merge_into) {
            return launch_history_norm_events(a, nt, sc.rec.get(), sc.stage.get<double>(), sc.scratch.get(), segments, merge_into, h->desc.n_entities, period,
                                              first_tick, n_samples, every, hs.ring, h->elem_size(), h->stream.get());
        },
        [&] { return norm_events_capture_args(a, nt); });
} SIXDOF_ABI_CATCH(err_of(h))

// How long and how often a predicate on an element, a difference or a squared vector length held, per condition and run.  One walk
// (and merge) launch covers all conditions, a unit is one (condition, run); the accumulator is the staging buffer, as for the norms.
int sixdof_history_dwell(sixdof_handle* h, const sixdof_dwell_condition* conditions, size_t n_conditions, uint32_t period, uint64_t first_tick,
                         uint64_t n_samples, uint64_t every, double* host_dst, uint32_t flags) try {
    if (!h) return SIXDOF_ERR_INVALID_ARGUMENT;
    History& hs = h->hist;
    History::TimeScan& sc = hs.dwell;
    const TimeScanSpec spec{"history_dwell", SIXDOF_DWELL_ASYNC, SIXDOF_DWELL_CONTINUE, SIXDOF_DWELL_HOLD, "SIXDOF_DWELL_CONTINUE",
                            "conditions, period, rows and rings", "SIXDOF_DWELL_SEGMENTS", dwell_segments, kDwellFields, &sc};
    const std::string who = spec.who;
    const bool hold = (flags & SIXDOF_DWELL_HOLD) != 0;
    const uint64_t n = h->desc.n_entities;
    const uint32_t nc = static_cast<uint32_t>(n_conditions);
    DwellArgs a{};
    return time_scan_read(
        h, spec, first_tick, n_samples, every, flags,
        [&](bool&) -> int {
            if (int rc = run_scan_checks(h, who, n_conditions, "conditions", SIXDOF_DWELL_MAX_CONDITIONS, period); rc != SIXDOF_OK) return rc;
            if (!conditions || (!hold && !host_dst)) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, who + ": null argument");
            for (size_t k = 0; k < n_conditions; k++) {
                const sixdof_dwell_condition& c = conditions[k];
                const std::string which = who + ": condition " + std::to_string(k);
                if (int rc = norm_probe_resolve(h, which, c.probe, period, a.c[k].probe); rc != SIXDOF_OK) return rc;
                if (const char* fault = dwell_condition_fault(c.kind, c.op, c.probe.count, c.lo, c.hi))
                    return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, which + ": " + fault + " (kind " + std::to_string(c.kind) + ", op " + std::to_string(c.op) + ")");
                a.c[k].lo = c.lo, a.c[k].hi = c.hi, a.c[k].kind = c.kind, a.c[k].op = c.op;
            }
            return SIXDOF_OK;
        },
        [&](StagedRead& rd, History::ScanState& next, std::vector<uint64_t>& units) -> int {
            units.push_back(n / period * n_conditions);
            rd.add_block(hold ? nullptr : host_dst, static_cast<size_t>(units[0]) * kDwellPlanes * sizeof(double));
            next.signature = {n_conditions, period};
            for (uint32_t k = 0; k < nc; k++) {
                const sixdof_dwell_condition& c = conditions[k];
                uint64_t lo, hi;
                std::memcpy(&lo, &c.lo, sizeof(lo)), std::memcpy(&hi, &c.hi, sizeof(hi));
                norm_probe_sign(c.probe, a.c[k].probe, next);
                next.signature.insert(next.signature.end(), {c.kind, c.op, lo, hi});
            }
            return SIXDOF_OK;
        },
        [&](const StagedRead&, size_t, uint64_t, uint32_t segments, bool merge_into) -> int {
            hipError_t e = launch_history_dwell(a, nc, sc.stage.get<double>(), sc.scratch.get(), segments, merge_into, n, period, first_tick, n_samples, every, hs.ring,
                                                h->elem_size(), h->stream.get());
            return e == hipSuccess ? int(SIXDOF_OK) : h->hip_fail(e, "history_dwell");
        });
} SIXDOF_ABI_CATCH(err_of(h))

int sixdof_download_column(sixdof_handle* h, uint64_t component_id) try {
    if (!h) return SIXDOF_ERR_INVALID_ARGUMENT;
    Column* c = h->col(component_id);
    if (!c) return h->fail(SIXDOF_ERR_COMPONENT_NOT_FOUND, "download_column: unknown component");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = scatter_back(h, c);
    if (rc != SIXDOF_OK) return rc;
    if (c->bytes) HIP_TRY(h, hipMemcpyAsync(c->host, c->dev.get(), c->bytes, hipMemcpyDeviceToHost, h->stream.get()));
    HIP_TRY(h, hipStreamSynchronize(h->stream.get()));
    return SIXDOF_OK;
} SIXDOF_ABI_CATCH(err_of(h))

// H2D of ONE bound column: an external write to a component (StepContext.write_component, copy_db_to_world's per-component copy,
// impeller2_server.rs:320-362) reaches the device without re-uploading — and so clobbering — the columns the host never downloaded.
int sixdof_upload_column(sixdof_handle* h, uint64_t component_id) try {
    if (!h) return SIXDOF_ERR_INVALID_ARGUMENT;
    Column* c = h->col(component_id);
    if (!c) return h->fail(SIXDOF_ERR_COMPONENT_NOT_FOUND, "upload_column: unknown component");
    if (!h->resident) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, "upload_column: nothing is resident yet (sixdof_upload first)");
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = upload_one(h, c); rc != SIXDOF_OK) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream.get()));
    if (component_id == h->id_accel) h->accel_is_host_data = true;
    return SIXDOF_OK;
} SIXDOF_ABI_CATCH(err_of(h))

bool graph_eligible(const sixdof_handle* h) {
    return (h->desc.flags & SIXDOF_FLAG_USE_GRAPH) && !(h->desc.flags & SIXDOF_FLAG_TIME_EACH_LAUNCH) && !h->hist.ring &&
           (h->custom_model.empty() || h->custom_tick_free) && h->model == 0 && !h->has_pair_op();
}

// Whether a batch of `n_ticks` opens with the accel-check launch: the first RK4 launch after an upload (step_rigid).
static bool opens_with_check(const sixdof_handle* h, uint64_t n_ticks) {
    return h->accel_is_host_data && h->desc.integrator == SIXDOF_INTEGRATOR_RK4 && n_ticks > 0;
}

// Whether the handle's launches may leave world_accel and force unwritten (StepParams::state_only): a built-in pipe without
// a history ring.  Inside one sixdof_step call nothing reads the two columns between launches — the host cannot look
// before the call returns, RK4 reads world_accel in the accel-check launch only — so every launch of a batch but the last
// overwrites them unread.  Launch i of a batch of L carries the flag iff i < L - 1 and it is not the accel-check launch:
// the LAST launch of every call stores all four columns, and after any call they hold what they always held.
static bool state_only_eligible(const sixdof_handle* h) {
    return !h->replay.state_only_off && !h->custom_launch && !h->hist.ring && h->model == 0 && !h->has_pair_op();
}

constexpr size_t kGraphCacheMax = 8;

// A chain's launches: kAll = every launch stores all four columns (handles that never use the flag), kStateOnly = every
// launch carries StepParams::state_only (more of the batch follows), kClosing = state-only launches and a last one that
// stores everything (the chain ends the batch).
enum class Chain : uint32_t { kAll = 0, kStateOnly = 1, kClosing = 2 };
static uint32_t graph_key(uint32_t len, Chain v) { return len << 2 | static_cast<uint32_t>(v); }

// An executable graph of `len` launches of the step kernel, cached per chain length and variant (Replay::key holds for all).
int ensure_graph(sixdof_handle* h, const StepParams& P, uint32_t len, Chain variant, hipGraphExec_t* out) {
    std::map<uint32_t, hipGraphExec_t>& graphs = h->replay.graphs;
    if (auto it = graphs.find(graph_key(len, variant)); it != graphs.end()) {
        *out = it->second;
        return SIXDOF_OK;
    }
    if (graphs.size() >= kGraphCacheMax) {   // many distinct batch lengths: keep the 32- and 128-launch chains (every variant), drop the rest
        for (auto g = graphs.begin(); g != graphs.end();) {
            if (g->first >> 2 == kGraphLen || g->first >> 2 == kGraphLong) { ++g; continue; }
            hipGraphExecDestroy(g->second);
            g = graphs.erase(g);
        }
    }
    StepParams Q = P;
    Q.state_only = variant == Chain::kAll ? 0u : 1u;
    hipGraph_t g = nullptr;
    HIP_TRY(h, hipStreamBeginCapture(h->stream.get(), hipStreamCaptureModeThreadLocal));
    hipError_t le = hipSuccess;
    for (uint32_t i = 0; i < len && le == hipSuccess; i++) {
        if (i + 1 == len && variant == Chain::kClosing) Q.state_only = 0;
        le = launch_any(h, Q);
    }
    hipError_t ce = hipStreamEndCapture(h->stream.get(), &g);
    if (le != hipSuccess) return h->hip_fail(le, "launch_step (capture)");
    if (ce != hipSuccess) return h->hip_fail(ce, "hipStreamEndCapture");
    hipGraphExec_t exec = nullptr;
    hipError_t ie = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
    hipGraphDestroy(g);
    if (ie != hipSuccess) return h->hip_fail(ie, "hipGraphInstantiate");
    (void)hipGraphUpload(exec, h->stream.get());   // move the one-off device-side setup out of the first replay
    graphs[graph_key(len, variant)] = exec;
    *out = exec;
    return SIXDOF_OK;
}

// One step of a plan's replay sequence: `times` replays of the `len`-launch chain `variant`.
struct ChainReplay {
    uint32_t len = 0;
    Chain variant = Chain::kAll;
    uint64_t times = 0;
    hipGraphExec_t graph = nullptr;
};

// The replays of batch plan `b`, in order, their graphs from the cache or captured now.  A chain that closes the batch
// (no eager launch, no remainder and no further replay after it) is the kClosing variant; on a handle that uses the flag
// every other chain is state-only throughout.  The one chain that is neither 32 nor 128 launches long (the tail) is
// looked up last, so a cache eviction it triggers (which keeps the 32- and 128-launch chains) drops none of the others.
static int ensure_plan_graphs(sixdof_handle* h, const StepParams& P, const BatchPlan& b, ChainReplay r[5]) {
    const ChainPlan& c = b.chains;
    const Chain v = state_only_eligible(h) ? Chain::kStateOnly : Chain::kAll;
    r[0] = {kGraphLen, v, c.open ? 1u : 0u};
    r[1] = {kGraphLong, v, c.n_long};
    r[2] = {kGraphLen, v, c.n_short};
    r[3] = {c.tail, v, c.tail ? 1u : 0u};
    r[4] = {};
    if (v == Chain::kStateOnly && c.launches() && c.launches() == b.full && !b.rem) {
        int last = 3;
        while (!r[last].times) last--;
        r[last].times--;
        r[4] = {r[last].len, Chain::kClosing, 1};
    }
    for (bool tail : {false, true})
        for (int i = 0; i < 5; i++) {
            if (!r[i].times || (r[i].len != kGraphLen && r[i].len != kGraphLong) != tail) continue;
            if (int rc = ensure_graph(h, P, r[i].len, r[i].variant, &r[i].graph); rc != SIXDOF_OK) return rc;
        }
    return SIXDOF_OK;
}

// ---- AQL chains ------------------------------------------------------------------------------------------------
// A graph-eligible batch of a built-in pipe is written into the process's own HSA queue as dispatch packets of the same
// kernel objects HIP launches (select_step), with argument blocks built ahead of the batch.  The launches are plan_batch's.

constexpr size_t kAqlSlotBytes = (sizeof(StepParams) + 255) / 256 * 256;
constexpr double kAqlStallS = 60.0;     // no packet of a chain started or finished for this long: the queue is stuck

// The packet run of one launch of `P` with `check` / `state_only` / `ticks` (its kernel and argument block, count 0), built
// on first use.  The argument blocks of the K-tick launches keep slots 0 (plain), 1 (accel check) and 2 (state-only) for
// as long as the parameters hold.  Any other block (a remainder, or a batch shorter than K: both close their batch, so
// neither is ever state-only) takes the next spare slot, evicting whichever block was there: a batch holds at most one
// such block (aql_batch), so no block a batch is about to run can be overwritten by its own later lookups, and nothing is
// in flight between two batches.
static bool aql_run(sixdof_handle* h, const StepParams& P, uint32_t check, uint32_t state_only, uint32_t ticks, aql::Run* out) {
    Replay& rp = h->replay;
    const uint64_t key = uint64_t(state_only) << 33 | uint64_t(check) << 32 | ticks;
    if (auto it = rp.aql_runs.find(key); it != rp.aql_runs.end()) return *out = it->second, true;
    uint32_t slot_index = state_only ? 2 : check;
    if (ticks != h->desc.ticks_per_launch) {
        slot_index = rp.aql_next_spare;
        rp.aql_next_spare = slot_index + 1 == kAqlSlots ? kAqlSpare0 : slot_index + 1;
        rp.aql_runs.erase(rp.aql_slot_key[slot_index]);
        rp.aql_slot_key[slot_index] = 0;
    }
    StepParams Q = P;
    Q.accel_in_check = check;
    Q.state_only = state_only;
    Q.n_ticks = ticks;
    Q.tick0 = Q.hist_slot0 = 0;   // read only by generated and history-ring pipes, which never take this path
    const StepKernel k = select_step(Q, h->desc.integrator, h->desc.dtype);
    if (!k.fn) return rp.aql_why = "no built-in kernel for this launch", false;
    aql::Run r;
    if (!aql::kernel_code(rp.aql_dev, k.fn, sizeof(StepParams), &r.code, &rp.aql_why)) return false;
    if (r.code.kernarg_align > 256) return rp.aql_why = "kernarg alignment above 256 bytes", false;
    char* slot = rp.aql_args.get<char>() + slot_index * kAqlSlotBytes;
    hipError_t e = hipMemcpy(slot, &Q, sizeof(Q), hipMemcpyHostToDevice);
    if (e != hipSuccess) return rp.aql_why = std::string("hipMemcpy (argument block): ") + hipGetErrorString(e), false;
    r.kernarg = slot;
    r.blocks = k.grid.x;
    rp.aql_runs[key] = r;
    if (slot_index >= kAqlSpare0) rp.aql_slot_key[slot_index] = key;
    return *out = r, true;
}

constexpr size_t kAqlRuns = 4;

// The runs of a batch planned by `b`: the accel-check launch, the state-only K-tick launches, the K-tick launches that
// store everything (one, and only when no remainder follows it, on a handle that uses the flag; else all of them), the
// remainder.  What the plan replays and the eager launches it leaves are the same packets.  Apart from the three K-tick
// blocks, the runs hold at most one block: a remainder needs n_ticks >= K, and then the check launch runs K ticks.
static bool aql_batch(sixdof_handle* h, const StepParams& P, const BatchPlan& b, aql::Run runs[kAqlRuns]) {
    const uint32_t K = h->desc.ticks_per_launch;
    const uint64_t closing = state_only_eligible(h) ? (b.full && !b.rem ? 1 : 0) : b.full;
    const uint64_t state_only = b.full - closing;
    if ((b.check_ticks && !aql_run(h, P, 1, 0, b.check_ticks, &runs[0])) || (state_only && !aql_run(h, P, 0, 1, K, &runs[1])) ||
        (closing && !aql_run(h, P, 0, 0, K, &runs[2])) || (b.rem && !aql_run(h, P, 0, 0, b.rem, &runs[3])))
        return false;
    runs[0].count = b.check_ticks ? 1 : 0;
    runs[1].count = state_only;
    runs[2].count = closing;
    runs[3].count = b.rem ? 1 : 0;
    return true;
}

enum class Path { kApollo, kPair, kAql, kRigid };   // kRigid: the step kernel through HIP, hipGraph replays or eager

struct Route {
    Path path;
    const char* why = nullptr;   // kRigid: why the batch is no AQL chain
    int rc = SIXDOF_OK;          // the step kernel's parameters could not be made: the step fails with this
    BatchPlan plan{};            // kAql, kRigid: the batch's launches
};

// The path of a batch of `n_ticks`: what sixdof_step runs, sixdof_step_path reports and the prepare calls build for.  For
// the step kernel, *P gets the batch's parameters (n_ticks = K) and the replay caches are keyed to them.  kAql has built
// the batch's packet runs into runs[]; when they cannot be built, aql_why says why, and this batch, like every later one,
// takes kRigid.  A handle whose chain faulted stays on kAql, where the step reports the fault.
static Route choose_path(sixdof_handle* h, uint64_t n_ticks, StepParams* P, aql::Run runs[kAqlRuns]) {
    if (h->model == 1) return {Path::kApollo};
    if (h->has_pair_op()) return {Path::kPair};
    Replay& rp = h->replay;
    const bool replay = graph_eligible(h);
    const char* why = nullptr;   // why the batch is no AQL chain
    if (rp.aql_off) why = "SIXDOF_AQL=0";
    else if (!replay) why = "not graph-eligible";
    else if (h->custom_launch) why = "generated pipe";
    else if (h->desc.flags & SIXDOF_FLAG_ASYNC_STEP) why = "ASYNC_STEP";
    else if (h->desc.n_entities == 0) why = "no rows";
    else if (!rp.aql_why.empty()) why = rp.aql_why.c_str();   // setup failed earlier: not retried
    else if (!rp.aql_fault.empty()) return {Path::kAql};
    else if (!h->resident) why = "columns not uploaded yet";
    if (!h->bound) return {Path::kRigid, why, SIXDOF_ERR_COMPONENT_NOT_FOUND};
    if (int rc = fill_step_params(h, P); rc != SIXDOF_OK) return {Path::kRigid, why ? why : h->err.c_str(), rc};
    const uint32_t K = h->desc.ticks_per_launch;
    P->n_ticks = K;
    if (replay) rp.rekey(*P);
    const BatchPlan plan = plan_batch(n_ticks, K, opens_with_check(h, n_ticks), replay);
    if (!why && !rp.aql_dev && (rp.aql_dev = aql::acquire(h->device, &rp.aql_why))) {   // the queue and the arena, once
        if (hipError_t e = rp.aql_args.alloc(kAqlSlots * kAqlSlotBytes); e != hipSuccess)
            rp.aql_why = std::string("hipMalloc: ") + hipGetErrorString(e);
    }
    if (!why && (!rp.aql_why.empty() || !aql_batch(h, *P, plan, runs))) why = rp.aql_why.c_str();
    return {why ? Path::kRigid : Path::kAql, why, SIXDOF_OK, plan};
}

// Builds what a batch of `n_ticks` replays ahead of it, so that no step call pays for it: its AQL argument blocks, or the
// hipGraphs of its chains (capture + instantiation).  Whether the batch opens with the accel-check launch the library
// cannot know (a warm-up batch may come first), so both shapes are built.
static int prepare_batch(sixdof_handle* h, const Route& r, const StepParams& P, uint64_t n_ticks) {
    if (r.path == Path::kAql && !h->replay.aql_fault.empty()) return SIXDOF_OK;   // the step reports the fault
    aql::Run runs[kAqlRuns];
    ChainReplay unused[5];
    for (bool check : {false, opens_with_check(h, n_ticks)}) {
        const BatchPlan b = plan_batch(n_ticks, h->desc.ticks_per_launch, check, true);
        if (r.path == Path::kAql) (void)aql_batch(h, P, b, runs);   // on failure the step takes the hipGraph path
        else if (int rc = ensure_plan_graphs(h, P, b, unused); rc != SIXDOF_OK) return rc;
    }
    if (r.path != Path::kAql) HIP_TRY(h, hipStreamSynchronize(h->stream.get()));
    return SIXDOF_OK;
}

// Builds what a first long batch replays (called when the columns become resident and when the batch shape changes): the
// blocks of the K-tick launches (a two-launch batch has all three), or the 32-launch chain that more of the batch follows.
int prepare_graph(sixdof_handle* h) {
    if (!h->bound || !graph_eligible(h)) return SIXDOF_OK;
    StepParams P;
    aql::Run runs[kAqlRuns];
    const Route r = choose_path(h, h->desc.ticks_per_launch, &P, runs);
    if (r.rc != SIXDOF_OK) return SIXDOF_OK;     // not steppable yet (columns missing): the step call will report it
    if (r.path == Path::kAql) return prepare_batch(h, r, P, 2 * uint64_t(h->desc.ticks_per_launch));
    hipGraphExec_t unused = nullptr;
    int rc = ensure_graph(h, P, kGraphLen, state_only_eligible(h) ? Chain::kStateOnly : Chain::kAll, &unused);
    if (rc == SIXDOF_OK) (void)hipStreamSynchronize(h->stream.get());
    return rc;
}

int sixdof_prepare_step(sixdof_handle* h, uint64_t n_ticks) try {
    if (!h) return SIXDOF_ERR_INVALID_ARGUMENT;
    if (!h->bound || !h->resident) return h->fail(SIXDOF_ERR_COMPONENT_NOT_FOUND, "prepare_step: upload the columns first");
    if (!graph_eligible(h)) return SIXDOF_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    StepParams P;
    aql::Run runs[kAqlRuns];
    const Route r = choose_path(h, n_ticks, &P, runs);
    return r.rc != SIXDOF_OK ? r.rc : prepare_batch(h, r, P, n_ticks);
} SIXDOF_ABI_CATCH(err_of(h))

const char* sixdof_step_path(sixdof_handle* h) try {
    if (!h) return "invalid handle";
    (void)hipSetDevice(h->device);
    StepParams P;
    aql::Run runs[kAqlRuns];
    const Route r = choose_path(h, h->desc.ticks_per_launch, &P, runs);   // as for a batch of one launch
    if (r.path == Path::kApollo) h->path = "apollo";
    else if (r.path == Path::kPair) h->path = "pair";
    else if (r.path == Path::kAql) h->path = h->replay.aql_fault.empty() ? "aql" : "aql (failed: " + h->replay.aql_fault + ")";
    else h->path = std::string(graph_eligible(h) ? "hipgraph: " : "eager: ") + r.why;
    return h->path.c_str();
} SIXDOF_ABI_CATCH_VALUE(err_of(h), nullptr)

// Pair effectors: one launch call per K ticks.  The multi-kernel path's batch is ONE pack launch, then fold + integrate
// per tick (the integrate kernel writes the next tick's pack rows); with a telemetry ring the batch is cut at every tick
// for the snapshot, the pack rows carry over all the same.
static int step_pair(sixdof_handle* h, uint64_t n_ticks, uint64_t* launches) {
    if (h->desc.dtype != SIXDOF_F64) return h->fail(SIXDOF_ERR_UNSUPPORTED, "step: pair effectors are f64 only");
    PairParams P;
    int rc = fill_pair_params(h, &P);
    if (rc != SIXDOF_OK) return rc;
    const char* no_small = std::getenv("SIXDOF_PAIR_SMALL");   // "0": force the multi-kernel path (tests)
    const bool custom = P.pair_kind == SIXDOF_EFF_EDGE_CUSTOM;
    bool small = P.n <= kPairSmallMax && !(no_small && no_small[0] == '0');   // small graphs: ticks_per_launch ticks per launch
    if (custom) {
        if (!h->pair_launch) return h->fail(SIXDOF_ERR_BACKEND, "step: custom pair op without sixdof_set_custom_pair");
        if (h->pair_only_small >= 0) small = h->pair_only_small == 1;
        if (small && P.n > kPairSmallMax)
            return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, "step: the pair object was generated for the one-launch small-graph kernel (<= " +
                           std::to_string(kPairSmallMax) + " rows) but the joined graph has " + std::to_string(P.n) + " rows");
    }
    const uint32_t K = h->hist.ring ? 1u : (small ? h->desc.ticks_per_launch : 1u << 20);
    // the integrate kernel leaves the next tick's pack rows (this call only: PairParams::packed); the built-in small-graph
    // kernel packs in-launch
    const bool sets_packed = custom || !small;
    for (uint64_t done = 0; done < n_ticks;) {
        const uint32_t k = static_cast<uint32_t>(std::min<uint64_t>(K, n_ticks - done));
        if (custom) {
            hipError_t e = static_cast<hipError_t>(h->pair_launch(&P, h->desc.integrator, k, small ? 1 : 0, h->stream.get(), launches));
            if (e != hipSuccess) return h->hip_fail(e, "custom pair launch");
        } else if (small) {
            hipError_t e = launch_pair_small(P, h->desc.integrator, k, h->stream.get(), launches);
            if (e != hipSuccess) return h->hip_fail(e, "launch_pair_small");
        } else {
            hipError_t e = launch_pair_ticks(P, h->desc.integrator, k, h->stream.get(), launches);
            if (e != hipSuccess) return h->hip_fail(e, "launch_pair_ticks");
        }
        done += k;
        if (sets_packed) P.packed = 1;
        if (int src = snapshot_tick_to_ring(h, h->tick + done); src != SIXDOF_OK) return src;
    }
    return SIXDOF_OK;
}

// The step kernel through HIP: K ticks per launch, the plan's chains replayed from hipGraphs (launch-bound regime: a
// 65,536-entity tick is a few microseconds of device time), the rest launched eagerly.
static int step_rigid(sixdof_handle* h, const StepParams& P, const BatchPlan& b, uint64_t n_ticks, uint64_t* launches) {
    const uint32_t K = h->desc.ticks_per_launch;
    const bool time_each = (h->desc.flags & SIXDOF_FLAG_TIME_EACH_LAUNCH) != 0;
    if (time_each) {
        const uint64_t need = 2 * b.launches();
        if (need > 8192) return h->fail(SIXDOF_ERR_INVALID_ARGUMENT, "step: TIME_EACH_LAUNCH supports <= 4096 launches per call");
        while (h->launch_events.size() < need) {
            Event e;
            HIP_TRY(h, hipEventCreate(e.out()));
            h->launch_events.push_back(std::move(e));
        }
    }
    // one eager launch of `ticks` ticks; every launch before it ran K ticks.  State-only unless it is the accel-check launch
    // or closes the batch (state_only_eligible).
    const bool may_skip = state_only_eligible(h);
    auto eager = [&](StepParams Q, uint32_t ticks) -> int {
        Q.n_ticks = ticks;
        Q.state_only = may_skip && !Q.accel_in_check && *launches + 1 < b.launches();
        Q.tick0 = Q.hist_slot0 = h->tick + *launches * K;
        if (time_each) HIP_TRY(h, hipEventRecord(h->launch_events[2 * *launches].get(), h->stream.get()));
        hipError_t e = launch_any(h, Q);
        if (e != hipSuccess) return h->hip_fail(e, "launch_step");
        if (time_each) HIP_TRY(h, hipEventRecord(h->launch_events[2 * *launches + 1].get(), h->stream.get()));
        ++*launches;
        return SIXDOF_OK;
    };
    if (n_ticks > 0) h->accel_is_host_data = false;
    if (b.check_ticks) {
        // First launch after an upload: the world_accel column holds whatever the host put there.  The reference's RK4
        // forms v_s = v0 + 0 * a_in on stage 0 (rk4.rs:96-100), so a non-finite row poisons that tick; this one launch
        // reads the column to do the same (step_kernel.hpp).  Every later a_in is this kernel's own output and is
        // already folded into v0.  A launch of its own, eager, so the replay graphs never carry the flag.
        StepParams P1 = P;
        P1.accel_in_check = 1;
        if (int rc = eager(P1, b.check_ticks); rc != SIXDOF_OK) return rc;
    }
    if (const ChainPlan& c = b.chains; c.launches()) {
        ChainReplay replays[5];
        if (int rc = ensure_plan_graphs(h, P, b, replays); rc != SIXDOF_OK) return rc;
        // a capture may just have happened after ev0 was recorded: re-record so the pair brackets real work only
        HIP_TRY(h, hipEventRecord(h->ev0.get(), h->stream.get()));
        for (const ChainReplay& r : replays)
            for (uint64_t i = 0; i < r.times; i++) HIP_TRY(h, hipGraphLaunch(r.graph, h->stream.get()));
        *launches += c.launches();
    }
    h->last.graph_launches = b.chains.launches();
    for (uint64_t i = b.chains.launches(); i < b.full; i++)
        if (int rc = eager(P, K); rc != SIXDOF_OK) return rc;
    return b.rem ? eager(P, b.rem) : SIXDOF_OK;
}

// The batch's packet runs as one AQL chain: step_rigid's launches, counted the same way, then a spin on the last packet.
static int step_aql(sixdof_handle* h, const BatchPlan& b, const aql::Run runs[kAqlRuns], uint64_t n_ticks, uint64_t* launches) {
    Replay& rp = h->replay;
    if (!rp.aql_fault.empty()) return h->fail(SIXDOF_ERR_BACKEND, rp.aql_fault);
    // the chain bypasses the HIP stream: let what was enqueued there (and on the null stream it waits for) finish first
    for (hipStream_t s : {h->stream.get(), static_cast<hipStream_t>(nullptr)}) {
        const hipError_t q = hipStreamQuery(s);
        if (q == hipErrorNotReady) HIP_TRY(h, hipStreamSynchronize(s));
        else if (q != hipSuccess) return h->hip_fail(q, "hipStreamQuery");
    }
    double device_ms = 0.0;
    if (!aql::run_chain(rp.aql_dev, runs, kAqlRuns, kAqlStallS, &device_ms, &rp.aql_fault))
        return h->fail(SIXDOF_ERR_BACKEND, rp.aql_fault);
    if (n_ticks > 0) h->accel_is_host_data = false;
    *launches = b.launches();
    h->last.graph_launches = b.chains.launches();
    h->last.kernel_device_ms = device_ms;
    return SIXDOF_OK;
}

int sixdof_step(sixdof_handle* h, uint64_t n_ticks, sixdof_timings* tm) try {
    if (!h) return SIXDOF_ERR_INVALID_ARGUMENT;
    if (!h->bound) return h->fail(SIXDOF_ERR_COMPONENT_NOT_FOUND, "step: no columns bound");
    HIP_TRY(h, hipSetDevice(h->device));
    const double t0 = now_ms();
    const bool async_step = (h->desc.flags & SIXDOF_FLAG_ASYNC_STEP) != 0;
    if (h->step_pending || h->prev_pending) {
        // asynchronous batches alternate between two event pairs, so the host may enqueue batch i+1 while batch i
        // still computes; the pair about to be re-recorded belongs to batch i-1 (long finished): read its time
        std::swap(h->ev0, h->evp0);
        std::swap(h->ev1, h->evp1);
        std::swap(h->step_pending, h->prev_pending);
        if (h->step_pending) {
            float ms_prev = 0.f;
            HIP_TRY(h, hipEventSynchronize(h->ev1.get()));
            if (hipEventElapsedTime(&ms_prev, h->ev0.get(), h->ev1.get()) == hipSuccess) h->last.kernel_device_ms = ms_prev;
            h->step_pending = false;
        }
    }
    if (h->hist.ring && h->copy.pending && h->copy.stream_hi >= h->copy.stream_lo && n_ticks) {
        // ticks tick+1 .. tick+n land in slots (t-1) % ring: hold the compute stream back only if that range reaches a
        // slot the copy stream may still be reading
        const uint64_t ring = h->hist.ring, in_flight = h->copy.stream_hi - h->copy.stream_lo + 1;
        const uint64_t a = history_slot(h->tick + 1, ring), b = history_slot(h->copy.stream_lo, ring);   // first slot written / first slot read
        const uint64_t gap_ab = (b + ring - a) % ring, gap_ba = (a + ring - b) % ring;
        const bool overlap = n_ticks + in_flight > ring || gap_ab < std::min<uint64_t>(n_ticks, ring) || gap_ba < in_flight;
        if (overlap) HIP_TRY(h, hipStreamWaitEvent(h->stream.get(), h->copy.ev_copied.get(), 0));
    }
    if (h->desc.integrator == SIXDOF_INTEGRATOR_NONE && (!h->custom_launch || h->model != 0 || h->has_pair_op()))
        return h->fail(SIXDOF_ERR_UNSUPPORTED, "step: SIXDOF_INTEGRATOR_NONE runs generated system programs only (sixdof_set_custom_pipe)");
    uint64_t launches = 0;
    StepParams P;
    aql::Run runs[kAqlRuns];
    const Route r = choose_path(h, n_ticks, &P, runs);
    if (r.rc != SIXDOF_OK) return r.rc;
    // an AQL chain waits for itself and times itself from its packets: no event pair on the HIP stream
    const bool aql = r.path == Path::kAql;
    if (!aql) HIP_TRY(h, hipEventRecord(h->ev0.get(), h->stream.get()));
    const int rc = aql                       ? step_aql(h, r.plan, runs, n_ticks, &launches)
                   : r.path == Path::kApollo ? step_apollo(h, n_ticks, &launches)
                   : r.path == Path::kPair   ? step_pair(h, n_ticks, &launches)
                                             : step_rigid(h, P, r.plan, n_ticks, &launches);
    if (rc != SIXDOF_OK) return rc;
    if (!aql) HIP_TRY(h, hipEventRecord(h->ev1.get(), h->stream.get()));
    if (!async_step && !aql) {
        // short batches finish in tens of microseconds: poll for that long before paying a blocking wait's wake-up
        const double spin_until = now_ms() + 0.25;
        hipError_t q = hipEventQuery(h->ev1.get());
        while (q == hipErrorNotReady && now_ms() < spin_until) q = hipEventQuery(h->ev1.get());
        if (q != hipSuccess) {
            (void)hipGetLastError();
            HIP_TRY(h, hipStreamSynchronize(h->stream.get()));
        }
        float ms0 = 0.f;
        hipEventElapsedTime(&ms0, h->ev0.get(), h->ev1.get());
        h->last.kernel_device_ms = ms0;
    }
    h->tick += n_ticks;  // increment_sim_tick (globals.rs:42-44), once per tick
    h->step_pending = async_step;
    h->last.kernel_invoke_ms = now_ms() - t0;
    h->last.launches = launches;
    h->last.ticks = n_ticks;
    h->last.kernel_sum_ms = 0.0;
    if ((h->desc.flags & SIXDOF_FLAG_TIME_EACH_LAUNCH) && !h->has_pair_op()) {
        for (uint64_t i = 0; i < launches && 2 * i + 1 < h->launch_events.size(); i++) {
            float one = 0.f;
            if (hipEventElapsedTime(&one, h->launch_events[2 * i].get(), h->launch_events[2 * i + 1].get()) == hipSuccess) h->last.kernel_sum_ms += one;
        }
    }
    if (tm) *tm = h->last;
    return SIXDOF_OK;
} SIXDOF_ABI_CATCH(err_of(h))

// ---- TickFn-compatible shim (cranelift_exec.rs:11,129-195) -----------------------------------------------------

static thread_local sixdof_handle* g_tick_handle = nullptr;

int sixdof_tick_bind(sixdof_handle* h) try {
    g_tick_handle = h;
    return SIXDOF_OK;
} SIXDOF_ABI_CATCH(err_of(h))

static void tick_slot_ids(const sixdof_handle* h, std::vector<uint64_t>* in, std::vector<uint64_t>* out) {
    // inputs: first-use order of `increment_sim_tick | six_dof(sys)` (system.rs:172-200); then effector columns
    *in = {h->id_tick, h->id_force, h->id_inertia, h->id_pos, h->id_dt, h->id_vel, h->id_accel};
    for (auto& o : h->ops)
        if (o.aux_component_id) in->push_back(o.aux_component_id);
    // outputs: every variable of the builder in ascending ComponentId (BTreeMap, system.rs:139-153)
    std::map<uint64_t, int> ordered;
    for (uint64_t id : *in) ordered[id] = 1;
    out->clear();
    for (auto& kv : ordered) out->push_back(kv.first);
}

static uint64_t slot_bytes(const sixdof_handle* h, uint64_t id) {
    if (id == h->id_tick || id == h->id_dt) return 8;
    const Column* c = h->col(id);
    return c ? c->bytes : 0;
}

int sixdof_tick_slots(const sixdof_handle* h, sixdof_slot* inputs, size_t in_cap, size_t* n_in, sixdof_slot* outputs,
                      size_t out_cap, size_t* n_out) try {
    if (!h || !n_in || !n_out) return SIXDOF_ERR_INVALID_ARGUMENT;
    std::vector<uint64_t> in, out;
    tick_slot_ids(h, &in, &out);
    *n_in = in.size();
    *n_out = out.size();
    if (in_cap < in.size() || out_cap < out.size())
        return h->fail(SIXDOF_ERR_VALUE_SIZE_MISMATCH, "tick_slots: buffer too small");
    for (size_t i = 0; inputs && i < in.size(); i++) inputs[i] = {in[i], slot_bytes(h, in[i])};
    for (size_t i = 0; outputs && i < out.size(); i++) outputs[i] = {out[i], slot_bytes(h, out[i])};
    return SIXDOF_OK;
} SIXDOF_ABI_CATCH(err_of(h))

void sixdof_tick(const uint8_t* const* inputs, uint8_t* const* outputs) try {
    sixdof_handle* h = g_tick_handle;
    if (!h || !h->bound || !inputs || !outputs) return;  // TickFn cannot fail (cranelift_exec.rs:163-165)
    if (hipSetDevice(h->device) != hipSuccess) return;
    std::vector<uint64_t> in, out;
    tick_slot_ids(h, &in, &out);
    uint64_t tick = 0;
    for (size_t i = 0; i < in.size(); i++) {
        if (in[i] == h->id_tick) std::memcpy(&tick, inputs[i], 8);
        else if (in[i] == h->id_dt) std::memcpy(&h->desc.simulation_time_step, inputs[i], 8);
        else if (Column* c = h->col(in[i])) {
            if (c->bytes) hipMemcpyAsync(c->dev.get(), inputs[i], c->bytes, hipMemcpyHostToDevice, h->stream.get());
            if (in[i] == h->id_accel) h->accel_is_host_data = true;   // a_in is host data on every TickFn call (rk4.rs:96-100)
            (void)gather_joined(h, c);
        }
    }
    h->tick = tick;
    const uint32_t k = h->desc.ticks_per_launch;
    h->desc.ticks_per_launch = 1;
    sixdof_step(h, 1, nullptr);
    h->desc.ticks_per_launch = k;
    for (size_t i = 0; i < out.size(); i++) {
        if (out[i] == h->id_tick) std::memcpy(outputs[i], &h->tick, 8);
        else if (out[i] == h->id_dt) std::memcpy(outputs[i], &h->desc.simulation_time_step, 8);
        else if (Column* c = h->col(out[i])) {
            scatter_back(h, c);
            if (c->bytes) hipMemcpyAsync(outputs[i], c->dev.get(), c->bytes, hipMemcpyDeviceToHost, h->stream.get());
        }
    }
    hipStreamSynchronize(h->stream.get());
} SIXDOF_ABI_CATCH_VALUE(err_of(g_tick_handle), )      // TickFn returns nothing: the message is on the bound handle

}  // extern "C"
