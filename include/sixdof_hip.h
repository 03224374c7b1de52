/*
 * sixdof_hip.h — C ABI of the MI355X-native 6DOF rigid-body integrator.
 *
 * This is the drop-in boundary for ONE path of elodin-sys/elodin: the `six_dof`
 * system (RK4 / semi-implicit) executed over ECS columns.  Every entry point
 * names the reference interface it replaces (paths relative to the reference
 * checkout).  Plain pointers and sizes only; no C++/torch types cross the ABI.
 *
 *   reference boundary                                        this header
 *   --------------------------------------------------------  -----------------------
 *   CraneliftExec::new            cranelift_exec.rs:54-127    sixdof_create + sixdof_bind_columns
 *   CraneliftExec::invoke_batch   cranelift_exec.rs:129-195   sixdof_step
 *   JaxExec H2D / D2H per batch   jax_exec.rs:130-177         sixdof_upload / sixdof_download
 *   TickFn(inputs**, outputs**)   cranelift_exec.rs:11        sixdof_tick (+ sixdof_tick_bind)
 *   ExecMetadata slot tables      exec.rs:17-29               sixdof_tick_slots
 *   Error -> PyErr                error.rs                    negative sixdof_status + sixdof_last_error
 *   ComponentId::new              impeller2/src/types.rs:39-44 sixdof_component_id
 *   validate_rates dt quantise    world_builder.rs:211-243    sixdof_quantize_time_step
 *   six_dof(time_step, sys, integrator)  six_dof.rs:161-203   sixdof_desc + sixdof_set_effectors
 *   GraphQuery edges              graph.rs:17-41,113-175      sixdof_set_edges
 *   JIT of user systems           cranelift_compile.rs:13-162 sixdof_set_custom_pipe / sixdof_set_custom_pair
 *   World / Column / spawn        world.rs:23-45,193-229      sixdof_world_* + sixdof_bind_world
 *   commit_world_head per batch   impeller2_server.rs:390-438 sixdof_download_async / _wait, sixdof_set_history
 *   failure detection / resume    (process exit, DB replay)   sixdof_count_nonfinite, sixdof_get/set_tick
 *   campaign fan-out / fan-in     monte-carlo/src/lib.rs:1066-1140,2083  sixdof_comm_*, sixdof_campaign_broadcast / _gather
 *
 * Column byte layout is the reference's (`World.host`, world.rs:23-45): row r of a
 * component occupies bytes [r*size, (r+1)*size), little-endian, row-major, rows in
 * spawn order, `entity_ids[r]` u64 LE.  The same bytes are kept resident in HBM.
 *
 * Threading: one handle = one GPU = one caller thread (mirrors the reference, where the
 * exec is moved once into the sim thread, cranelift_exec.rs:31-51).  Handles on
 * different GPUs may be driven from different threads.  Nothing throws across the ABI.
 */
#ifndef SIXDOF_HIP_H
#define SIXDOF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIXDOF_ABI_VERSION 2   /* 2: sixdof_timings.graph_launches, sixdof_apollo_tables.ticks_per_telemetry, effector kinds 10-11 */

typedef struct sixdof_handle sixdof_handle;

/* 0 = ok, negative = error.  Mirrors nox-py `Error` (libs/nox-py/src/error.rs). */
typedef enum sixdof_status {
    SIXDOF_OK = 0,
    SIXDOF_ERR_INVALID_ARGUMENT = -1,
    SIXDOF_ERR_COMPONENT_NOT_FOUND = -2,  /* Error::ComponentNotFound   */
    SIXDOF_ERR_VALUE_SIZE_MISMATCH = -3,  /* Error::ValueSizeMismatch   */
    SIXDOF_ERR_BACKEND = -4,              /* Error::CraneliftBackend(String) analogue: HIP runtime failure */
    SIXDOF_ERR_NO_DEVICE = -5,
    SIXDOF_ERR_UNSUPPORTED = -6,
    SIXDOF_ERR_ENTITY_MISMATCH = -7,      /* Body columns do not share one entity-id vector */
    SIXDOF_ERR_TIME_TRAVEL = -8,          /* elodin-db Error::TimeTravel: a sample older than the pair's last one */
    /* The exception barrier (csrc/abi_guard.hpp): a C++ exception never unwinds into the caller's frames (Rust `extern "C"`,
     * cranelift_exec.rs:11,163-165).  Every allocating entry point catches, leaves the text in *_last_error and returns: */
    SIXDOF_ERR_OUT_OF_MEMORY = -9,        /* std::bad_alloc / std::length_error: a host allocation failed (absurd row count?) */
    SIXDOF_ERR_INTERNAL = -10             /* any other exception: Error::Unknown / PyErr analogue (error.rs:12-51) */
} sixdof_status;

/* integrator/mod.rs:7-10 */
typedef enum sixdof_integrator {
    SIXDOF_INTEGRATOR_RK4 = 0,
    SIXDOF_INTEGRATOR_SEMI_IMPLICIT = 1,
    /* no six_dof stage: a pipe of per-entity systems only (`World.build(system)`, Query::map query.rs:504-545);
     * valid only with a generated program (sixdof_set_custom_pipe); world_accel / force pass through unchanged */
    SIXDOF_INTEGRATOR_NONE = 2
} sixdof_integrator;

/* Arithmetic type of the state columns.  The reference six_dof is f64 only
 * (six_dof.rs:12-14,133-135); F32 is an extension for BASELINE config 5. */
typedef enum sixdof_dtype {
    SIXDOF_F64 = 0,
    SIXDOF_F32 = 1
} sixdof_dtype;

/* impeller2 PrimType subset used by this path */
typedef enum sixdof_prim {
    SIXDOF_PRIM_F64 = 0,
    SIXDOF_PRIM_U64 = 1,
    SIXDOF_PRIM_F32 = 2
} sixdof_prim;

/*
 * Effector pipeline: the `sys` argument of six_dof(), i.e. what runs between
 * clear_forces and calc_accel on every integrator stage (six_dof.rs:184-203).
 * The reference takes arbitrary JAX; this backend takes a list of built-in ops
 * applied in pipe order.  Each op cites the example effector it restates.
 */
typedef enum sixdof_effector_kind {
    /* F += [tau(3), f(3)] = p[0..6), world frame.  test_all.py:342-364 constant_force */
    SIXDOF_EFF_CONST_WRENCH = 1,
    /* f += (p[0],p[1],p[2]) * mass.  examples/ball/sim.py:57-59 */
    SIXDOF_EFF_UNIFORM_GRAVITY = 2,
    /* tau += q * aux[i][0..3)  (body-frame torque column).  examples/apollo-lander/sim.py:396-398 */
    SIXDOF_EFF_BODY_TORQUE = 3,
    /* f += q * aux[i][0..3)  (body-frame force column).  examples/apollo-lander/sim.py:391-394 */
    SIXDOF_EFF_BODY_FORCE = 4,
    /* F = Force(linear = f + drag) with wind = aux[i][0..3), p = {Cd, rho, area}.
     * NOTE: clears the torque, like the reference.  examples/ball/sim.py:96-116 */
    SIXDOF_EFF_BALL_DRAG = 5,
    /* edge_fold over sixdof_set_edges(): acc.f -= p[0]*M*m*r/|r|^3, r = a-b (p[0] = G).
     * Result REPLACES Force for source rows.  examples/three-body/main.py:56-78 */
    SIXDOF_EFF_EDGE_GRAVITY_NEWTON = 6,
    /* edge_fold: acc.f += (p[0]*ma*mb*inv3)*r, r = b-a, inv = 1/sqrt(r.r+p[1]) (p = {K, eps}).
     * examples/n-body/sim.py:344-369 */
    SIXDOF_EFF_EDGE_GRAVITY_SOFTENED = 7,
    /* Same fold as 7 over the complete graph (for i: for j != i, ascending), without
     * materialising edges.  examples/n-body/sim.py:333-337 spawn order */
    SIXDOF_EFF_ALLPAIRS_GRAVITY_SOFTENED = 8,
    /* edge_fold whose fold function is generated code (sixdof_set_custom_pair); never passed to
     * sixdof_set_effectors directly.  graph.rs:177-282 edge_fold with an arbitrary `fn` */
    SIXDOF_EFF_EDGE_CUSTOM = 9,
    /* per-entity ops again (kinds 6..9 are the pair ops): */
    /* tau += aux[i][0..3)  (world-frame torque column): `force + el.SpatialForce(torque=c)` with c a per-entity
     * component, the shape of every effector that applies an externally computed load; it is also what a
     * teacher-forced replay of a recorded `force` column (scripts/ci/baseline/cube-sat-csv) feeds the step */
    SIXDOF_EFF_WORLD_TORQUE = 10,
    /* f += aux[i][0..3)  (world-frame force column).  Same pattern, linear half */
    SIXDOF_EFF_WORLD_FORCE = 11
} sixdof_effector_kind;
/* kinds 6..9 fold over edges / pairs; every other kind is a per-entity op */
#define SIXDOF_EFF_IS_PAIR(k) ((k) >= SIXDOF_EFF_EDGE_GRAVITY_NEWTON && (k) <= SIXDOF_EFF_EDGE_CUSTOM)

typedef struct sixdof_effector_op {
    int32_t kind;               /* sixdof_effector_kind */
    int32_t reserved;
    uint64_t aux_component_id;  /* per-entity [n,3] f64 column for kinds 3,4,5,10,11; else 0 */
    double p[6];
} sixdof_effector_op;

typedef struct sixdof_desc {
    uint32_t struct_size;        /* = sizeof(sixdof_desc) */
    int32_t device_ordinal;      /* HIP device */
    int32_t integrator;          /* sixdof_integrator */
    int32_t dtype;               /* sixdof_dtype */
    uint64_t n_entities;         /* size of the joined Body entity set; 0 = take it from the bound columns */
    double simulation_time_step; /* globals column value (ns-quantised, see sixdof_quantize_time_step) */
    double time_step;            /* six_dof(time_step=...) override, used iff has_time_step */
    int32_t has_time_step;
    uint32_t ticks_per_launch;   /* ticks fused into one kernel launch (>=1). 1 = every tick
                                    materialises all output columns in HBM (reference tick semantics);
                                    K>1 = the reference's ticks_per_telemetry batch, state in registers */
    uint32_t flags;              /* SIXDOF_FLAG_* */
    uint32_t reserved;
} sixdof_desc;

#define SIXDOF_FLAG_USE_GRAPH 1u /* run sixdof_step batches of >= 4 launches as a pre-built chain: for a built-in pipe,
                                    dispatch packets written into the library's own HSA queue (SIXDOF_AQL=0 at creation:
                                    off; sixdof_step_path tells); otherwise captured hipGraphs (chains of 32 + one chain of
                                    the remainder, cached per length).
                                    On every path (eager launches too), a launch of a built-in pipe without a history ring
                                    that another launch of the same sixdof_step call follows stores world_pos and world_vel
                                    only: the last launch of every call stores world_accel and force as well, so after any
                                    call the four columns hold what they always held (SIXDOF_STATE_ONLY=0 at creation:
                                    every launch stores all four, for A/B runs) */
#define SIXDOF_FLAG_TIME_EACH_LAUNCH 2u /* profiling: bracket every launch of sixdof_step with its own HIP
                                           event pair (<= 4096 launches per call; disables graph replay) */
#define SIXDOF_FLAG_ASYNC_STEP 4u /* sixdof_step only enqueues and returns (no stream sync): pair it with
                                     sixdof_download_async so the telemetry copy of batch i overlaps batch i+1;
                                     kernel_device_ms then reports the previous finished batch.  sixdof_sync joins. */

/* One ECS column as the reference holds it (world.rs:26-30 + ExecSlotMetadata exec.rs:17-22). */
typedef struct sixdof_column {
    uint64_t component_id;       /* sixdof_component_id("world_pos") ... */
    int32_t prim_type;           /* sixdof_prim */
    uint32_t ndim;               /* 0 (scalar), 1 */
    uint64_t dims[2];            /* e.g. {7} */
    uint64_t n_rows;
    const uint64_t* entity_ids;  /* [n_rows] */
    void* host_ptr;              /* caller-owned row-major bytes; borrowed until destroy/rebind */
} sixdof_column;

/* profile.rs TickTimings analogue (ms) */
typedef struct sixdof_timings {
    double h2d_upload_ms;
    double kernel_invoke_ms;   /* host wall time of the step call incl. stream sync */
    double d2h_download_ms;
    double kernel_device_ms;   /* device time of the launches of the last step: HIP events on the handle's stream, or for
                                  an AQL chain the first dispatch's start to the last one's end (starts later than the
                                  event, which also holds the wait in front of the first launch) */
    uint64_t launches;         /* kernel launches issued by the last step */
    uint64_t ticks;
    double kernel_sum_ms;      /* SIXDOF_FLAG_TIME_EACH_LAUNCH: sum of the per-launch event times (no gaps) */
    uint64_t graph_launches;   /* how many of `launches` ran from a pre-built chain (SIXDOF_FLAG_USE_GRAPH): an AQL chain
                                  or a captured hipGraph */
} sixdof_timings;

typedef struct sixdof_slot {
    uint64_t component_id;
    uint64_t bytes;
} sixdof_slot;

/* download masks */
#define SIXDOF_COL_WORLD_POS 1u
#define SIXDOF_COL_WORLD_VEL 2u
#define SIXDOF_COL_WORLD_ACCEL 4u
#define SIXDOF_COL_FORCE 8u
#define SIXDOF_COL_INERTIA 16u
#define SIXDOF_COL_ALL 31u

uint32_t sixdof_abi_version(void);
/* FNV-1a-64(name) & ~(1<<63): impeller2/src/types.rs:39-44 */
uint64_t sixdof_component_id(const char* name);
/* Duration::from_secs_f64(1/rate).as_secs_f64(): world_builder.rs:221, world.rs:185-191 */
double sixdof_quantize_time_step(double simulation_rate_hz);
int sixdof_device_count(void);

int sixdof_create(const sixdof_desc* desc, sixdof_handle** out);
void sixdof_destroy(sixdof_handle* h);
const char* sixdof_last_error(const sixdof_handle* h); /* h may be NULL: last create error */

/* Same-size columns keep their device copies.  A failed call (after the argument check) leaves the handle UNBOUND: every
 * column bound so far owns valid device memory or none, step / upload / download refuse, and a later bind succeeds. */
int sixdof_bind_columns(sixdof_handle* h, const sixdof_column* cols, size_t n_cols);
int sixdof_set_effectors(sixdof_handle* h, const sixdof_effector_op* ops, size_t n_ops);
/* Edges as (from entity id, to entity id) in spawn order; resolved to row indices against the
 * bound Body entity ids (query.rs:599-621 gathers by constant u32 indices).  The new tables are built next to the old
 * ones and swapped in last: a failed call leaves the handle's edges (sixdof_get_edge_rows, what the step reads) unchanged. */
int sixdof_set_edges(sixdof_handle* h, const uint64_t* from_ids, const uint64_t* to_ids, size_t n_edges);
/* Join tables: row of joined entity j inside column `component_id` — the constant u32 gather indices the
 * reference bakes at compile time (query.rs:599-621).  six_dof runs over the INTERSECTION of the Body columns'
 * entity ids in ascending id order (query.rs:136-208); when every Body column already is that set the order is
 * the columns' own (fast path query.rs:673,702) and rows[j] = j.  rows == NULL just returns the joined count. */
int sixdof_get_join_rows(const sixdof_handle* h, uint64_t component_id, uint32_t* rows, size_t cap, size_t* n_out);
/* Read back the resolved u32 row-index tables (bit-exact integer parity surface). */
int sixdof_get_edge_rows(const sixdof_handle* h, uint32_t* src_rows, uint32_t* dst_rows, size_t cap, size_t* n_out);

int sixdof_upload(sixdof_handle* h);
int sixdof_step(sixdof_handle* h, uint64_t n_ticks, sixdof_timings* timings /* may be NULL */);
/* SIXDOF_FLAG_USE_GRAPH: capture (and cache) the launch chains a later sixdof_step(h, n_ticks) replays, without stepping —
 * the one-off cost CraneliftExec::new pays at build time (cranelift_exec.rs:54-127), kept out of the first timed batch. */
int sixdof_prepare_step(sixdof_handle* h, uint64_t n_ticks);
/* Which path the next sixdof_step batch takes, and why not the AQL chain when it does not: "aql", "hipgraph: <why>",
 * "eager: <why>", "pair" or "apollo".  Sets the AQL chain up when the columns are resident.  Valid until the next call. */
const char* sixdof_step_path(sixdof_handle* h);
int sixdof_download(sixdof_handle* h, uint32_t column_mask);
/* Telemetry commit without the per-batch stall (the step either side of the path: commit_world_head after
 * every batch, impeller2_server.rs:390-438; JaxExec blocks on copy_to_host there, jax_exec.rs:150-178).
 * download_async snapshots the selected columns on the compute stream (device-to-device, microseconds) and
 * copies the snapshot into the bound host buffers on a second stream; the host buffers are page-locked on
 * first use (hipHostRegister) so the copy is a real DMA.  The next sixdof_step may be issued immediately.
 * download_wait blocks until the host buffers hold that snapshot.  One snapshot in flight: a second
 * download_async first waits (on the device) for the previous copy to have left the snapshot buffers.
 * The copy stream and its two events are created on first use, all three or none: a call that fails there (or anywhere
 * else) leaves nothing pending and the next call starts afresh. */
int sixdof_download_async(sixdof_handle* h, uint32_t column_mask);
int sixdof_download_wait(sixdof_handle* h);
int sixdof_sync(sixdof_handle* h);   /* both streams idle */
int sixdof_get_tick(const sixdof_handle* h, uint64_t* tick);
int sixdof_set_tick(sixdof_handle* h, uint64_t tick);
int sixdof_set_ticks_per_launch(sixdof_handle* h, uint32_t k);
int sixdof_set_flags(sixdof_handle* h, uint32_t flags);
/* Device-resident column (reference byte layout) for zero-copy consumers; NULL if unknown. */
void* sixdof_device_column(sixdof_handle* h, uint64_t component_id);
/* hipStream_t the handle launches on, as an opaque pointer */
void* sixdof_stream(sixdof_handle* h);

/* TickFn-compatible entry (cranelift_exec.rs:11): upload -> 1 tick -> download through the
 * slot tables below.  sixdof_tick_bind selects the handle for the calling thread. */
int sixdof_tick_bind(sixdof_handle* h);
void sixdof_tick(const uint8_t* const* inputs, uint8_t* const* outputs);
/* inputs: order of first use; outputs: ascending ComponentId (system.rs:139-153). */
int sixdof_tick_slots(const sixdof_handle* h, sixdof_slot* inputs, size_t in_cap, size_t* n_in,
                      sixdof_slot* outputs, size_t out_cap, size_t* n_out);

/* ---- health / profiling ------------------------------------------------------------------------------------------
 * Per-rollout failure sentinel (a campaign's replacement for "the sim process exited non-zero",
 * libs/monte-carlo/src/lib.rs:2083-2379): counts joined rows whose world_pos or world_vel holds a NaN/Inf and,
 * if `row_flags` is non-NULL, writes one byte per joined row (1 = non-finite). */
int sixdof_count_nonfinite(sixdof_handle* h, uint64_t* count, uint8_t* row_flags /* [n] or NULL */);
/* Timings of the most recent upload / step / download (profile.rs:14-59 phases). */
int sixdof_last_timings(const sixdof_handle* h, sixdof_timings* out);

/* ---- host-side ECS column store: the `World` of libs/nox-py/src/world.rs:23-45,174-229 ---------------------------
 * Per component a growing row-major buffer + the entity id of each row, rows in spawn order, ids sequential,
 * entity 0 = "Globals" (tick u64, simulation_time_step f64).  Pure host code: needs no GPU. */
typedef struct sixdof_world sixdof_world;
sixdof_world* sixdof_world_create(void);
void sixdof_world_destroy(sixdof_world* w);
const char* sixdof_world_last_error(const sixdof_world* w);
uint64_t sixdof_world_spawn(sixdof_world* w);                 /* World::spawn: next sequential EntityId */
uint64_t sixdof_world_entity_len(const sixdof_world* w);
/* World::insert_with_id for one component: append `row` (n_bytes = prod(dims) * sizeof(prim)) and the entity id. */
int sixdof_world_insert(sixdof_world* w, uint64_t entity, const char* component, int prim_type, const uint64_t* dims,
                        uint32_t ndim, const void* row, size_t n_bytes);
/* World::column_by_id: a view (pointers stay valid until the next insert into that component). */
int sixdof_world_column(sixdof_world* w, uint64_t component_id, sixdof_column* out);
size_t sixdof_world_components(const sixdof_world* w, uint64_t* ids, size_t cap); /* ascending ComponentId */
/* validate_rates + set_globals (world_builder.rs:211-243): telemetry_rate_hz = 0 means "same as simulation". */
int sixdof_world_set_rates(sixdof_world* w, double simulation_rate_hz, double telemetry_rate_hz);
double sixdof_world_time_step(const sixdof_world* w);
uint64_t sixdof_world_ticks_per_telemetry(const sixdof_world* w);
uint64_t sixdof_world_tick(const sixdof_world* w);
void sixdof_world_advance_tick(sixdof_world* w, uint64_t n);
/* Bind every 1-D f64/f32 component column of the world to the backend handle (CraneliftExec::new walks
 * world.column_by_id the same way, cranelift_exec.rs:101-106).  Follow with sixdof_upload. */
int sixdof_bind_world(sixdof_handle* h, sixdof_world* w);

/* ---- the commit path's hand-off: per (entity, component) pair one time series ------------------------------------------
 * What commit_world_head_for_world (libs/nox-py/src/impeller2_server.rs:398-438) writes after every batch and
 * copy_db_to_world (:320-364) reads back before the next: PairId = ComponentId::from_pair(entity, component)
 * (impeller2/src/types.rs:54-59), a series = an index of i64 microsecond timestamps + the samples' bytes
 * (libs/db/src/time_series.rs:201-230: a push older than the last timestamp is SIXDOF_ERR_TIME_TRAVEL).  The database
 * behind it (files, subscriptions, wire protocol) is out of scope; pure host code, needs no GPU. */
typedef struct sixdof_sink sixdof_sink;
uint64_t sixdof_pair_id(const char* entity, const char* component);               /* ComponentId::from_pair */
sixdof_sink* sixdof_sink_create(void);
void sixdof_sink_destroy(sixdof_sink* s);
const char* sixdof_sink_last_error(const sixdof_sink* s);
int sixdof_sink_register(sixdof_sink* s, uint64_t pair_id, uint32_t elem_bytes, const char* name);
int sixdof_sink_push(sixdof_sink* s, uint64_t pair_id, int64_t timestamp_us, const void* buf, uint32_t bytes);   /* TimeSeries::push_buf */
uint64_t sixdof_sink_sample_count(const sixdof_sink* s, uint64_t pair_id);
size_t sixdof_sink_pairs(const sixdof_sink* s, uint64_t* ids, size_t cap);        /* ascending PairId */
int sixdof_sink_latest(const sixdof_sink* s, uint64_t pair_id, int64_t* timestamp_us, void* out, uint32_t bytes);
/* the sample with the greatest timestamp <= timestamp_us (past the last write: the latest; before the first:
 * SIXDOF_ERR_COMPONENT_NOT_FOUND) — StepContext.read_component(timestamp=), elodin.pyi:63-88 */
int sixdof_sink_at(const sixdof_sink* s, uint64_t pair_id, int64_t timestamp_us, int64_t* found_us, void* out, uint32_t bytes);
/* the two append logs of a pair, as the database would persist them (valid until the next push) */
int sixdof_sink_series(const sixdof_sink* s, uint64_t pair_id, const int64_t** timestamps, const uint8_t** data, uint64_t* n,
                       uint32_t* elem_bytes);
void sixdof_sink_truncate(sixdof_sink* s);
/* commit_world_head for one column: row i of `rows` ([n_rows, row_bytes], e.g. a bound host column after sixdof_download /
 * sixdof_download_wait) -> the series of pair_ids[i] (0 or unregistered: skipped, like an entity without metadata). */
int sixdof_sink_commit_rows(sixdof_sink* s, const uint64_t* pair_ids, const void* rows, uint32_t n_rows, uint32_t row_bytes,
                            int64_t timestamp_us);
/* copy_db_to_world for one column: latest samples -> rows; *changed = 1 when a byte differed (follow with sixdof_upload). */
int sixdof_sink_copy_to_rows(const sixdof_sink* s, const uint64_t* pair_ids, void* rows, uint32_t n_rows, uint32_t row_bytes,
                             int* changed);

/* ---- effector front-end: run-time generated pipes -------------------------------------------------------------
 * The reference JIT-compiles whatever effector graph the user wrote (cranelift_compile.rs:13-162).  The analogue
 * here: elodin_amd/codegen.py turns an effector pipe written against a jax.numpy-like tracer into HIP source that
 * instantiates the SAME fused step kernel (csrc/step_kernel.hpp) with the user's code as its effector stage,
 * builds it with hipcc for gfx950 and hands the shared object to this call.  `aux_component_ids` name the bound
 * per-entity columns the generated code uses, in the order it indexes them: first the read-only effector
 * columns (row width 1..3, <= 4), then — for whole programs `pre | six_dof(effectors) | post` — the component
 * columns its systems read AND write (row width 1..64 — a small matrix component is its row-major flattening —, <= 128 columns; fetch them back with sixdof_download_column).
 * A WINDOW column (a wide component such as the rocket example's 480 x 3 sample buffer, examples/rocket/main.py:91-98)
 * is bound like any other ([n, rows*width] elements) but stays in HBM, in the layout the generated object was built for: entity-major
 * (the reference's rows; small executors) or ELEMENT-major — buffer[e * n + entity] for e < rows*width, so that lane-adjacent
 * entities read adjacent addresses; executors of 32,768 entities or more —, used as a ring whose head
 * (physical index of the oldest row) lives in a hidden [n,1] column `<name>#head` — transpose + un-rotate after a download
 * (elodin_amd/exec.py HipExec.component does).  The generated object exports the row width it was built for per column; sixdof_step refuses columns bound
 * with another width.  A program may hold stand-alone folds between its systems (graph.rs:239-361): the generated launch
 * entry then issues a chain of kernels per tick (systems | fold | systems | six_dof | ...) over the same columns; the fold's
 * scratch rows are one more program column `<out>#fold<k>`.  Replaces the built-in op list (sixdof_set_effectors) for the
 * per-entity path.  An object built from a whole-world StableHLO tick with one lane per entity (cranelift_compile.rs:47-68's module,
 * `python -m elodin_amd.stablehlo`, manifest "rows_per_world") exchanges data between the entities of a world inside the
 * wavefront and exports the rows a world occupies; a handle whose n_entities is not a multiple of it is refused with
 * SIXDOF_ERR_INVALID_ARGUMENT. */
int sixdof_set_custom_pipe(sixdof_handle* h, const char* so_path, const uint64_t* aux_component_ids, size_t n_aux);
/* Same idea for GraphQuery.edge_fold (graph.rs:177-282) with a user-written fold function over
 * (acc: Force, a: (WorldPos, Inertia), b: (WorldPos, Inertia)): the generated object instantiates the pair kernels
 * (csrc/pair_kernel.hpp) with that function.  Appends the fold as the LAST op of the pipe set by
 * sixdof_set_effectors (per-entity built-in ops before it are kept); edges come from sixdof_set_edges. */
int sixdof_set_custom_pair(sixdof_handle* h, const char* so_path);
/* The edges of fold stage `fold_index` (order of the stages in the program) of a generated program whose fold kernels read
 * their edges from device memory (codegen: fold_tables="device"; such an object exports sixdof_custom_fold_count /
 * sixdof_custom_fold_info / sixdof_custom_set_fold_table, an object without them has its edges baked in).  Ids are resolved
 * to rows like sixdof_set_edges does; for a program generated for replicas (count x stride rows) they name entities of
 * replica 0.  The library builds the CSR by source in spawn order (sixdof_build_fold_table), splits the sources of a fold that
 * may be regrouped at out-degree 64 (one wave per long source, one lane per other source), checks every row, uploads on the
 * handle's stream and hands the table to the object.  May be called again between batches with any other edge list: the old
 * table is released once the stream has drained, and captured replays are dropped.  Rows that stop being sources keep their
 * last `out` value.  Until every such fold stage has a table sixdof_step returns SIXDOF_ERR_UNSUPPORTED.  Errors (nothing is
 * installed then): no generated program / a baked object -> SIXDOF_ERR_UNSUPPORTED; fold_index out of range, a fold over a
 * complete graph, more than 2^32 - 1 edges, a row outside the handle (replica 0) -> SIXDOF_ERR_INVALID_ARGUMENT; an unknown
 * entity id -> SIXDOF_ERR_COMPONENT_NOT_FOUND. */
int sixdof_set_fold_edges(sixdof_handle* h, uint32_t fold_index, const uint64_t* from_ids, const uint64_t* to_ids, size_t n_edges);
/* Pure host (no device): the table sixdof_set_fold_edges uploads, from ROW pairs.  Sources ascending, each source's targets
 * in the order given; with wave_min_degree > 0 the sources of out-degree below it come first (*n_lane of them), the others
 * behind, ascending inside each range.  out_src and out_dst hold n_edges values, out_start n_edges + 1; the table uses
 * *n_src, *n_src + 1 and n_edges of them.  A row >= row_limit or more than 2^32 - 1 edges: SIXDOF_ERR_INVALID_ARGUMENT. */
int sixdof_build_fold_table(const uint32_t* src_rows, const uint32_t* dst_rows, size_t n_edges, uint32_t row_limit,
                            uint32_t wave_min_degree, uint32_t* out_src, uint32_t* out_start, uint32_t* out_dst,
                            uint32_t* n_src, uint32_t* n_lane);

/* ---- telemetry: device-side history ring (the commit step either side of the path) ------------------------
 * The reference commits every output column to its DB after each batch (exec.rs:110-172,
 * impeller2_server.rs:390-438) and `exec.history()` reads it back.  With a ring enabled, sixdof_step writes
 * world_pos / world_vel / world_accel / force of EVERY tick into slot (tick-1) % ring_ticks of a device ring
 * (reference row layout, one contiguous [n,w] block per tick and column) from inside the fused kernel, so
 * ticks_per_launch > 1 no longer drops intermediate ticks.  With a generated program installed
 * (sixdof_set_custom_pipe) every component column of the program is recorded the same way and can be read
 * back by its component id.  Worlds stepped by the pair (edge_fold / all-pairs) kernels or by a rollout model are
 * recorded too: with a ring enabled they run one tick per launch and the four output columns are copied into the
 * tick's slot on the device (the model's own columns are not recorded).  ring_ticks = 0 disables and frees the ring.
 * The previous ring is freed FIRST (rings can be gigabytes).  A failed call, a component ring's allocation included,
 * leaves NO ring: every ring buffer is freed and the history calls answer as before the first sixdof_set_history. */
int sixdof_set_history(sixdof_handle* h, uint32_t ring_ticks);
/* Copy the [n,w] block of `component_id` as it was after `tick` ticks into host_dst.  Fails with
 * SIXDOF_ERR_INVALID_ARGUMENT if that tick is not (or no longer) in the ring. */
int sixdof_history_read(sixdof_handle* h, uint64_t component_id, uint64_t tick, void* host_dst);
/* Stream a run of recorded ticks to the host without stalling the stepper: the [n_ticks, n, w] blocks of
 * world_pos / world_vel / world_accel / force for ticks first_tick .. first_tick + n_ticks - 1 are copied, on the
 * copy stream, into host_dst[0..3] (a NULL entry skips that column; buffers are page-locked on first use).  Returns
 * once the copies are enqueued; sixdof_download_wait blocks until they have landed.  With SIXDOF_FLAG_ASYNC_STEP and a
 * ring of at least two batches the copy of batch i overlaps the compute of batch i+1: a later sixdof_step only waits
 * (on the device) when it is about to overwrite ring slots that are still being read.  The host buffers must stay
 * allocated until sixdof_sync, which also releases their page locks.  A failed call: the copy lane as for
 * sixdof_download_async (whole or absent); copies already enqueued may still land, so the buffers stay allocated until
 * sixdof_sync all the same; the ring is untouched and the call may be repeated. */
int sixdof_history_stream(sixdof_handle* h, uint64_t first_tick, uint64_t n_ticks, void* const host_dst[4]);

/* ---- watch lists: time series of chosen (entity, component) pairs out of the ring ----------------------------
 * What exec.history("e1.x"), a plot or the commit sink wants is a handful of pairs over time, often at a lower rate than
 * the simulation's — not every row of every tick.  A watch names the components and the entities once; a read gathers
 * their rows out of the ring on the device and moves m rows per sample to the host, not n.
 *
 * sixdof_set_watch: watchable components are the ones sixdof_history_read accepts (world_pos / world_vel / world_accel /
 * force and the non-window component columns of a generated program; anything else: SIXDOF_ERR_COMPONENT_NOT_FOUND).
 * Entity ids are resolved to rows of the joined Body set, in the order given; duplicates are allowed; an id outside the
 * join is SIXDOF_ERR_ENTITY_MISMATCH.  A failed call leaves the previous watch as it was.  0 components and 0 entities
 * clear the watch.  Independent of sixdof_set_history (either order, any later ring size); sixdof_bind_columns drops it. */
int sixdof_set_watch(sixdof_handle* h, const uint64_t* component_ids, size_t n_components, const uint64_t* entity_ids,
                     size_t n_entities);
#define SIXDOF_WATCH_ASYNC 1u
/* Read n_samples samples of every watched pair: sample j is the state after tick first_tick + j * every.  host_dst[k]
 * receives component k (the order of sixdof_set_watch) as [n_entities][n_samples][w_k]: one contiguous series per pair.
 * flags = 0: returns when the data is in host_dst.  SIXDOF_WATCH_ASYNC: returns once the gather and the copies are
 * enqueued (the copies on the copy stream, host_dst page-locked on first use); sixdof_download_wait blocks until they
 * have landed, and the buffers must stay allocated until sixdof_sync, as for sixdof_history_stream.  Either way the ring
 * is read on the compute stream, so a later sixdof_step may overwrite the slots without waiting for the copy.
 * n_samples = 0 is a no-op.  SIXDOF_ERR_INVALID_ARGUMENT, with nothing copied: no watch, no ring, every = 0, or a
 * sampled tick that is not (or no longer) in the ring.  A call that fails in the runtime leaves the watch and the ring as
 * they were; if the staging buffer could not be grown there is none (size 0) and the next read allocates it again; the
 * copy lane as for sixdof_download_async.  host_dst of a failed asynchronous read stays allocated until sixdof_sync. */
int sixdof_watch_read(sixdof_handle* h, uint64_t first_tick, uint64_t n_samples, uint64_t every, void* const host_dst[],
                      uint32_t flags);

/* ---- ring envelopes: the dispersion of ALL rows over time ------------------------------------------------------
 * What a dispersion plot or a go/no-go table of a campaign wants per tick and component element is how many runs are still
 * finite, their minimum, maximum, mean and spread — five numbers, reduced on the device, not n rows.
 *
 * For sample j (the state after tick first_tick + j * every), component k (the ones sixdof_history_read accepts; anything
 * else: SIXDOF_ERR_COMPONENT_NOT_FOUND) and group g < period, the rows r with r % period == g are reduced per element c < w_k.
 * period = 1: all rows; period = E: entity e of every run of a campaign whose runs are E consecutive rows.  host_dst[k]
 * receives [n_samples][period][5][w_k] doubles, the five in the order count, min, max, mean, m2:
 *   count   elements that are finite (non-finite elements are skipped, never propagated; count < rows / period shows them)
 *   min max mean   over those elements;  m2 = sum (x - mean)^2 over them (variance = m2 / count).  count = 0: all four NaN.
 * Accumulated in f64 whatever the handle's dtype.  No floating-point atomics; the launch geometry and merge order depend on
 * (n, w_k, period) only, so the values of one (tick, component) are bit-identical whichever range, `every`, component list or
 * flags read them.
 * flags = 0: returns when the data is in host_dst.  SIXDOF_ENVELOPE_ASYNC: the rules of SIXDOF_WATCH_ASYNC — the copies go on the
 * copy stream, sixdof_download_wait blocks until they have landed, host_dst stays allocated (and page-locked) until
 * sixdof_sync.  Either way the ring is read on the compute stream: a later sixdof_step may overwrite the slots at once.
 * n_samples = 0 is a no-op.  SIXDOF_ERR_INVALID_ARGUMENT, with nothing copied: no ring, every = 0, period = 0, a row count that
 * is no multiple of period, period * w_k above 512 (the bins one block of the kernel keeps apart), a sampled tick that is
 * not (or no longer) in the ring, unknown flags, a null buffer.  A call that fails in the runtime leaves the ring as it was; a
 * staging or partial buffer that could not be grown is absent (size 0) and the next call allocates it again. */
#define SIXDOF_ENVELOPE_ASYNC 1u
int sixdof_history_envelope(sixdof_handle* h, const uint64_t* component_ids, size_t n_components, uint64_t first_tick,
                            uint64_t n_samples, uint64_t every, uint32_t period, double* const host_dst[], uint32_t flags);

/* ---- ring quantiles: the percentile band of ALL rows over time -----------------------------------------------------
 * Mean and spread summarise a skewed dispersion, or one with a few diverging runs, poorly; what a campaign's reader wants of
 * touchdown velocity or propellant margin is p1 / p50 / p99 per tick — order statistics, selected on the device, exactly.
 *
 * Samples, components and groups are sixdof_history_envelope's: sample j is the state after tick first_tick + j * every, group
 * g < period the rows r with r % period == g, reduced per element c < w_k.  The ranks are the exact rationals
 * rank_num[i] / rank_den (1 <= rank_den, rank_num[i] <= rank_den, 1 <= n_ranks <= SIXDOF_QUANTILE_MAX_RANKS; duplicates and
 * any order are allowed).  With m the number of finite elements of a group (non-finite elements are skipped) and
 * x(0) <= ... <= x(m-1) those elements in ascending order,
 *   lo_i = floor(num_i * (m - 1) / den),  hi_i = ceil(num_i * (m - 1) / den)     in unsigned 64-bit integer arithmetic;
 * no floating-point rank arithmetic is used.  host_dst[k] receives [n_samples][period][1 + 2 * n_ranks][w_k] doubles:
 *   plane 0          m
 *   plane 1 + 2 * i  x(lo_i)
 *   plane 2 + 2 * i  x(hi_i)         m = 0: plane 0 is 0 and the rank planes are NaN.
 * Every value is an element of the ring converted to double (exact for an f32 handle): nothing is interpolated or rounded on
 * the device, so a value is bit-identical whichever range, `every`, component list, rank list or flags read it.  The order is
 * the total order of the sign-magnitude bit pattern: -0.0 sorts below +0.0.  A radix select, most significant byte first, over
 * integer keys: integer atomics only, 9 reads of a tick's block for f64 and 5 for f32, never a sort.
 * flags = 0: returns when the data is in host_dst.  SIXDOF_QUANTILE_ASYNC: the rules of SIXDOF_WATCH_ASYNC — the copies go on the
 * copy stream, sixdof_download_wait blocks until they have landed, host_dst stays allocated (and page-locked) until
 * sixdof_sync.  Either way the ring is read on the compute stream: a later sixdof_step may overwrite the slots at once.
 * n_samples = 0 is a no-op.  SIXDOF_ERR_INVALID_ARGUMENT, with nothing copied: no ring, every = 0, period = 0, a row count that
 * is no multiple of period, period * w_k above 512 (the envelope's limit), n_ranks of 0 or above 16, rank_den = 0, a numerator
 * above the denominator, a null rank pointer, a sampled tick that is not (or no longer) in the ring, unknown flags, a null
 * buffer.  A call that fails in the runtime leaves the ring as it was; a staging or scratch buffer that could not be grown is
 * absent (size 0) and the next call allocates it again. */
#define SIXDOF_QUANTILE_ASYNC 1u
#define SIXDOF_QUANTILE_MAX_RANKS 16
int sixdof_history_quantiles(sixdof_handle* h, const uint64_t* component_ids, size_t n_components, uint64_t first_tick,
                             uint64_t n_samples, uint64_t every, uint32_t period, const uint32_t* rank_num, uint32_t rank_den,
                             size_t n_ranks, double* const host_dst[], uint32_t flags);

/* ---- ring extremes: every row collapsed across time ------------------------------------------------------------------
 * What a campaign's results table wants per run is peak dynamic pressure and when, apogee and when, the lowest altitude, the tick
 * at which a run went non-finite — per row, collapsed across time, reduced on the device: six numbers per element, once.
 *
 * Samples and components are sixdof_history_envelope's: sample j is the state after tick first_tick + j * every, components are
 * the ones sixdof_history_read accepts (anything else: SIXDOF_ERR_COMPONENT_NOT_FOUND); an id may appear more than once.  For
 * component k, row r < n and element c < w_k, host_dst[k] receives [6][n][w_k] doubles, plane-major:
 *   plane 0  count             samples at which the element is finite
 *   plane 1  min               the smallest finite value
 *   plane 2  tick_min          the EARLIEST sampled tick that holds it
 *   plane 3  max               the largest finite value
 *   plane 4  tick_max          the EARLIEST sampled tick that holds it
 *   plane 5  first_nonfinite   the earliest sampled tick at which the element is not finite; 0: none
 * The order is sixdof_history_quantiles': the total order of the sign-magnitude bit pattern, -0.0 below +0.0, and "holds it" means
 * bit-equal.  count = 0: min and max are NaN, their ticks 0.  Ticks are counts of completed ticks as the handle counts them, as
 * doubles; tick 0 is never in the ring, so 0 means "none"; a range whose last sampled tick is 2^53 or more is refused.  Every
 * value is an element of the ring converted to double (exact for an f32 handle).  No floating-point arithmetic and no atomics:
 * a later sample replaces an extreme only when strictly smaller or larger, a rule that is exact and associative in time order,
 * so the result is bit-identical however the range is cut into time segments (SIXDOF_EXTREMES_SEGMENTS in the environment
 * forces a count; 0 or unset: the library's choice), launches or calls.
 * SIXDOF_EXTREMES_HOLD: reduce and keep the result in the device accumulator (the call's staging buffer, freed with the ring);
 * nothing is delivered, host_dst is ignored.  SIXDOF_EXTREMES_CONTINUE: merge into the accumulator the previous successful call
 * left instead of starting afresh — how a run longer than the ring is reduced batch by batch with nothing crossing the link until
 * the last call.  Accepted only if the previous call succeeded with the same component ids in the same order, ring bases, widths
 * and row count are unchanged, no sixdof_set_history or sixdof_bind_columns came since, and first_tick is above the last tick
 * accumulated; otherwise SIXDOF_ERR_INVALID_ARGUMENT and the accumulator stays as it was.
 * SIXDOF_EXTREMES_ASYNC: the rules of SIXDOF_WATCH_ASYNC — the copies go on the copy stream, sixdof_download_wait blocks until
 * they have landed, host_dst stays allocated (and page-locked) until sixdof_sync.  Either way the ring is read on the compute
 * stream: a later sixdof_step may overwrite the slots at once, and a ring one batch deep is enough.
 * n_samples = 0 is a no-op that leaves the accumulator alone.  SIXDOF_ERR_INVALID_ARGUMENT, with nothing copied and the
 * accumulator as it was: no ring, every = 0, a sampled tick that is not (or no longer) in the ring, unknown flags, a null
 * component_ids, a null buffer without SIXDOF_EXTREMES_HOLD.  A call that fails in the runtime leaves the ring as it was and the
 * accumulator invalid: the next SIXDOF_EXTREMES_CONTINUE is refused, a fresh call works; a staging or scratch buffer that could
 * not be grown is absent (size 0) and the next call allocates it again. */
#define SIXDOF_EXTREMES_ASYNC    1u
#define SIXDOF_EXTREMES_CONTINUE 2u
#define SIXDOF_EXTREMES_HOLD     4u
#define SIXDOF_EXTREMES_PLANES   6
int sixdof_history_extremes(sixdof_handle* h, const uint64_t* component_ids, size_t n_components, uint64_t first_tick,
                            uint64_t n_samples, uint64_t every, double* const host_dst[], uint32_t flags);

/* ---- ring events: the first threshold crossing of every run and the state there ------------------------------------------
 * What a campaign's results table asks most often: at what tick did this run reach a condition — touchdown, apogee, burn-out,
 * leaving a corridor — and what was its state at that tick.  The tick differs per run and the ring is overwritten batch by batch,
 * so event and state are found and captured on the device, in the call that sees the event.
 *
 * A run is `period` consecutive rows (n_entities % period == 0; runs = n_entities / period).  A trigger reads element `element`
 * of component `component_id` in row run * period + group of every run.  Its predicate is x op level: an IEEE compare of the
 * ring's element, widened to double (exact for an f32 handle), against a finite level, so -0.0 equals +0.0.  A non-finite sample
 * is skipped as if it had not been sampled: it neither holds nor fails and is never a "before" sample.  SIXDOF_EVENT_LEVEL: the
 * event is the earliest finite sample at which the predicate holds.  SIXDOF_EVENT_CROSSING: the earliest finite sample at which it
 * holds and the previous finite sample did not; a predicate that holds from the first sample on never fires.
 *
 * Samples are the ticks first_tick, first_tick + every, ... (n_samples of them), all in the ring.  event_dst is
 * [n_triggers][SIXDOF_EVENTS_PLANES][runs] doubles, plane-major: the event tick (0: none), the element's value at it (NaN: none),
 * the tick of the finite sample before it (0: none — also where a LEVEL event fell on the first finite sample) and that sample's
 * value (NaN: none).  capture_dst[k] is [n_triggers][n_entities][w_k] doubles: every row of component capture_ids[k] at the event
 * tick of the row's run for that trigger, NaN where the run has no event; n_captures = 0 reports the events only.  Ticks are
 * exact in doubles: a range whose last sampled tick is 2^53 or more is refused.  No floating-point arithmetic beyond the compare
 * and the widening and no atomics: the rule is exact and associative in time order, so every output is bit-identical however the
 * range is cut into time segments (SIXDOF_EVENTS_SEGMENTS in the environment forces a count; 0 or unset: the library's choice),
 * launches or calls.
 * SIXDOF_EVENTS_HOLD: reduce and keep the result in the device accumulator (the records and the call's staging buffer, freed
 * with the ring); nothing is delivered, event_dst and capture_dst are ignored.  SIXDOF_EVENTS_CONTINUE: merge into the
 * accumulator the previous successful call left instead of starting afresh; a capture taken by an earlier call stays.  Accepted
 * only if the previous call succeeded with the same triggers field for field, the same capture ids in the same order and the
 * same period, ring bases, widths and row count are unchanged, no sixdof_set_history or sixdof_bind_columns came since, and
 * first_tick is above the last tick accumulated; otherwise SIXDOF_ERR_INVALID_ARGUMENT and the accumulator stays as it was.
 * SIXDOF_EVENTS_ASYNC: the rules of SIXDOF_WATCH_ASYNC.  Either way the ring is read on the compute stream: a later sixdof_step
 * may overwrite the slots at once, and a ring one batch deep is enough.
 * n_samples = 0 is a no-op that leaves the accumulator alone.  SIXDOF_ERR_INVALID_ARGUMENT, with nothing copied and the
 * accumulator as it was: no ring, every = 0, a sampled tick that is not (or no longer) in the ring or is 2^53 or more, unknown
 * flags, a null triggers, a null capture_ids with n_captures > 0, a null event_dst, capture_dst or buffer without
 * SIXDOF_EVENTS_HOLD, n_triggers = 0 or above SIXDOF_EVENTS_MAX_TRIGGERS, period = 0 or not dividing n_entities, group >= period,
 * element >= the component's width, an unknown op or mode, a level that is not finite.  A trigger or capture component the ring
 * does not record: SIXDOF_ERR_COMPONENT_NOT_FOUND.  A call that fails in the runtime leaves the ring as it was and the
 * accumulator invalid, as for sixdof_history_extremes. */
typedef struct sixdof_event_trigger {   /* 32 bytes */
    uint64_t component_id;
    uint32_t element, group, op, mode;
    double level;
} sixdof_event_trigger;
#define SIXDOF_EVENT_LT 0u
#define SIXDOF_EVENT_LE 1u
#define SIXDOF_EVENT_GT 2u
#define SIXDOF_EVENT_GE 3u
#define SIXDOF_EVENT_LEVEL    0u
#define SIXDOF_EVENT_CROSSING 1u
#define SIXDOF_EVENTS_ASYNC    1u
#define SIXDOF_EVENTS_CONTINUE 2u
#define SIXDOF_EVENTS_HOLD     4u
#define SIXDOF_EVENTS_PLANES   4
#define SIXDOF_EVENTS_MAX_TRIGGERS 8
int sixdof_history_events(sixdof_handle* h, const sixdof_event_trigger* triggers, size_t n_triggers, const uint64_t* capture_ids,
                          size_t n_captures, uint32_t period, uint64_t first_tick, uint64_t n_samples, uint64_t every,
                          double* event_dst, double* const capture_dst[], uint32_t flags);

/* ---- ring norms: per-run extremes of a vector's length or of a separation -------------------------------------------------
 * Apogee and perigee are extremes of |r|, peak speed of |v|, peak tumble rate of |omega|, the drift of a quaternion from unit
 * length of |q|, the miss distance of chaser and target the smallest |r_a - r_b| and when: extremes over time of a scalar derived
 * from several elements, possibly of two rows of a run.  sixdof_history_extremes looks at one element of one row; this reader
 * forms the scalar on the device before the same rule sees it.
 *
 * A run is `period` consecutive rows (n_entities % period == 0; runs = n_entities / period).  Probe A reads elements element ..
 * element + count - 1 of component `component_id` in row run * period + group of every run; with SIXDOF_NORM_MINUS, B reads
 * elements minus_element .. minus_element + count - 1 of `minus_component_id` (which may equal component_id) in row run * period +
 * minus_group, otherwise the three minus_ fields are not read.  For each probe, run and sampled tick the value is the SQUARED
 * Euclidean norm s, in f64, in this fixed order: d_e = a_e (or a_e - b_e with SIXDOF_NORM_MINUS), s = d_0 * d_0, then s = s + d_e *
 * d_e for e = 1 .. count - 1.  Every ring element is widened to double first (exact for an f32 handle), and the code is compiled
 * without FMA contraction, so the library, its host twin and a plain restatement round alike, bit for bit.  A sample is finite
 * exactly when s is finite: any non-finite input gives a non-finite s (squares are non-negative, nothing cancels), and an s that
 * OVERFLOWS from finite inputs counts as non-finite too.  s then goes through the rule of sixdof_history_extremes unchanged.
 *
 * Samples are the ticks first_tick, first_tick + every, ... (n_samples of them), all in the ring.  host_dst is
 * [n_probes][SIXDOF_NORMS_PLANES][runs] doubles, plane-major:
 *   plane 0  count             samples at which s is finite
 *   plane 1  min_sq            the smallest finite s
 *   plane 2  tick_min          the EARLIEST sampled tick that holds it
 *   plane 3  max_sq            the largest finite s
 *   plane 4  tick_max          the EARLIEST sampled tick that holds it
 *   plane 5  first_nonfinite   the earliest sampled tick at which s is not finite; 0: none
 * count = 0: min_sq and max_sq are NaN, their ticks 0.  Ticks are exact in doubles: a range whose last sampled tick is 2^53 or
 * more is refused.  The rule is exact and associative in time order and there are no atomics, so every output is bit-identical
 * however the range is cut into time segments (SIXDOF_NORMS_SEGMENTS in the environment forces a count; 0 or unset: the
 * library's choice), launches or calls.  The square root is left to the caller.
 * SIXDOF_NORMS_HOLD: reduce and keep the result in the device accumulator (the call's staging buffer, freed with the ring);
 * nothing is delivered, host_dst is ignored.  SIXDOF_NORMS_CONTINUE: merge into the accumulator the previous successful call left
 * instead of starting afresh.  Accepted only if the previous call succeeded with the same probes field for field and the same
 * period, ring bases, widths and row count are unchanged, no sixdof_set_history or sixdof_bind_columns came since, and first_tick
 * is above the last tick accumulated; otherwise SIXDOF_ERR_INVALID_ARGUMENT and the accumulator stays as it was.
 * SIXDOF_NORMS_ASYNC: the rules of SIXDOF_WATCH_ASYNC.  Either way the ring is read on the compute stream: a later sixdof_step
 * may overwrite the slots at once, and a ring one batch deep is enough.
 * n_samples = 0 is a no-op that leaves the accumulator alone.  SIXDOF_ERR_INVALID_ARGUMENT, with nothing copied and the
 * accumulator as it was: no ring, every = 0, a sampled tick that is not (or no longer) in the ring or is 2^53 or more, unknown
 * flags, a null probes, a null host_dst without SIXDOF_NORMS_HOLD, n_probes = 0 or above SIXDOF_NORMS_MAX_PROBES, count = 0 or
 * above SIXDOF_NORM_MAX_COUNT, element + count (with SIXDOF_NORM_MINUS also minus_element + count) above the component's width,
 * group (minus_group) >= period, unknown probe flags, period = 0 or not dividing n_entities.  A component the ring does not
 * record: SIXDOF_ERR_COMPONENT_NOT_FOUND.  A call that fails in the runtime leaves the ring as it was and the accumulator
 * invalid, as for sixdof_history_extremes. */
typedef struct sixdof_norm_probe {     /* 40 bytes */
    uint64_t component_id;             /* A: elements element .. element+count-1 of row run*period+group */
    uint64_t minus_component_id;       /* B, read only with SIXDOF_NORM_MINUS; may equal component_id */
    uint32_t element, minus_element, group, minus_group;
    uint32_t count;                    /* 1 .. SIXDOF_NORM_MAX_COUNT (4: a quaternion) */
    uint32_t flags;                    /* 0 or SIXDOF_NORM_MINUS */
} sixdof_norm_probe;
#define SIXDOF_NORM_MINUS 1u
#define SIXDOF_NORM_MAX_COUNT 4
#define SIXDOF_NORMS_ASYNC 1u
#define SIXDOF_NORMS_CONTINUE 2u
#define SIXDOF_NORMS_HOLD 4u
#define SIXDOF_NORMS_PLANES 6
#define SIXDOF_NORMS_MAX_PROBES 8
int sixdof_history_norms(sixdof_handle* h, const sixdof_norm_probe* probes, size_t n_probes, uint32_t period,
                         uint64_t first_tick, uint64_t n_samples, uint64_t every, double* host_dst, uint32_t flags);

/* ---- ring norm events: the first crossing of a vector's length or of a separation per run, and the state there -------------
 * On a spherical or orbital world the conditions are lengths: touchdown or entry interface is |r| <= R + h, leaving a sphere of
 * influence |r| >= r_soi, a keep-out sphere or conjunction |r_chaser - r_target| < d, a speed or tumble-rate limit |v| > v_max or
 * |omega| > omega_max, loss of quaternion normalisation |q| > 1 + eps.  sixdof_history_events reads one element;
 * sixdof_history_norms keeps only the extremes of a norm.  This reader puts the norms' value under the events' rule.
 *
 * A run is `period` consecutive rows (n_entities % period == 0; runs = n_entities / period).  For each trigger, run and sampled
 * tick the value is s, exactly the SQUARED norm sixdof_history_norms forms of `probe` (every ring element widened to double, f64,
 * left to right, no FMA contraction).  A sample is finite exactly when s is: an s that overflows from finite inputs is non-finite
 * and therefore SKIPPED as the events skip a non-finite sample — it neither holds nor fails and is never a "before" sample.  The
 * predicate is the IEEE compare s op level_sq against the SQUARED level: no square root and no other arithmetic on the device.
 * SIXDOF_EVENT_LEVEL and SIXDOF_EVENT_CROSSING as for sixdof_history_events.
 *
 * Samples are the ticks first_tick, first_tick + every, ... (n_samples of them), all in the ring.  event_dst is
 * [n_triggers][SIXDOF_NORM_EVENTS_PLANES][runs] doubles, plane-major: the event tick (0: none), s at it (NaN: none), the tick of
 * the finite sample before it (0: none — also where a LEVEL event fell on the first finite sample) and s at that sample (NaN:
 * none).  capture_dst[k] is [n_triggers][n_entities][w_k] doubles: every row of component capture_ids[k] at the event tick of
 * the row's run for that trigger, NaN where the run has no event; n_captures = 0 reports the events only.  Ticks are exact in
 * doubles: a range whose last sampled tick is 2^53 or more is refused.  The rule is exact and associative in time order and there
 * are no atomics, so every output is bit-identical however the range is cut into time segments (SIXDOF_NORM_EVENTS_SEGMENTS in
 * the environment forces a count; 0 or unset: the library's choice), launches or calls.  The square roots are left to the caller.
 * SIXDOF_NORM_EVENTS_HOLD, SIXDOF_NORM_EVENTS_CONTINUE and SIXDOF_NORM_EVENTS_ASYNC behave as SIXDOF_EVENTS_HOLD, _CONTINUE and
 * _ASYNC: a continuing call rewrites only the captures of the runs whose event it saw, and is accepted only if the previous call
 * succeeded with the same triggers field for field (level_sq compared by its bits), the same capture ids in the same order and
 * the same period, ring bases, widths and row count are unchanged, no sixdof_set_history or sixdof_bind_columns came since, and
 * first_tick is above the last tick accumulated; otherwise SIXDOF_ERR_INVALID_ARGUMENT and the accumulator stays as it was.
 * n_samples = 0 is a no-op that leaves the accumulator alone.  SIXDOF_ERR_INVALID_ARGUMENT, with nothing copied and the
 * accumulator as it was: everything sixdof_history_events refuses for range, flags, buffers, n_triggers, period, op and mode,
 * everything sixdof_history_norms refuses for a probe, and a level_sq that is not finite or is below 0.  A probe or capture
 * component the ring does not record: SIXDOF_ERR_COMPONENT_NOT_FOUND.  A call that fails in the runtime leaves the ring as it was
 * and the accumulator invalid, as for sixdof_history_extremes. */
typedef struct sixdof_norm_trigger {   /* 56 bytes */
    sixdof_norm_probe probe;           /* as for sixdof_history_norms */
    double level_sq;                   /* finite, >= 0: the SQUARED level */
    uint32_t op, mode;                 /* SIXDOF_EVENT_LT .. SIXDOF_EVENT_GE; SIXDOF_EVENT_LEVEL or SIXDOF_EVENT_CROSSING */
} sixdof_norm_trigger;
#define SIXDOF_NORM_EVENTS_ASYNC    1u
#define SIXDOF_NORM_EVENTS_CONTINUE 2u
#define SIXDOF_NORM_EVENTS_HOLD     4u
#define SIXDOF_NORM_EVENTS_PLANES   4
#define SIXDOF_NORM_EVENTS_MAX_TRIGGERS 8
int sixdof_history_norm_events(sixdof_handle* h, const sixdof_norm_trigger* triggers, size_t n_triggers, const uint64_t* capture_ids,
                               size_t n_captures, uint32_t period, uint64_t first_tick, uint64_t n_samples, uint64_t every,
                               double* event_dst, double* const capture_dst[], uint32_t flags);

/* ---- ring dwell: per run, how long and how often a condition held -------------------------------------------------------------
 * The event readers answer WHEN something first happened, the extremes and the norms WHAT the extreme was.  A results table asks
 * as often HOW LONG and HOW OFTEN: the time above a dynamic-pressure or load limit, how many times a vehicle left its corridor
 * and whether it was still outside at the end, how long chaser and target stayed inside a keep-out sphere, the longest unbroken
 * stretch with |omega| above a tumble limit and when it began, the share of a flight spent in an altitude band.
 *
 * A run is `period` consecutive rows (n_entities % period == 0; runs = n_entities / period).  A condition is a probe — the struct
 * of sixdof_history_norms, read the same way — a kind, an op and two levels.  SIXDOF_DWELL_ELEMENT: probe.count must be 1, and the
 * value of a sample is the signed scalar v = a_0, or a_0 - b_0 with SIXDOF_NORM_MINUS: every ring element widened to double first
 * (exact for an f32 handle), one subtraction, no FMA contraction.  SIXDOF_DWELL_NORM_SQ: v is exactly the SQUARED norm s that
 * sixdof_history_norms forms of the probe, and lo and hi are SQUARED levels, not below 0.  The predicate is an IEEE compare:
 * SIXDOF_EVENT_LT .. SIXDOF_EVENT_GE: v op lo, and hi must be 0; SIXDOF_DWELL_INSIDE: lo <= v && v <= hi; SIXDOF_DWELL_OUTSIDE:
 * v < lo || v > hi; both with lo <= hi.  Levels are finite.  A sample is finite exactly when v is (an overflowing difference or
 * square is not); a non-finite sample is skipped as the events skip it: it neither holds nor fails, and a stretch continues
 * across it.  Nothing stops early: every sample counts.
 *
 * Samples are the ticks first_tick, first_tick + every, ... (n_samples of them), all in the ring.  host_dst is
 * [n_conditions][SIXDOF_DWELL_PLANES][runs] doubles, plane-major.  Ticks are counts of completed ticks, so 0 means "none";
 * lengths are counted in finite samples:
 *   plane 0   count           finite samples
 *   plane 1   held            finite samples at which the predicate holds
 *   plane 2   entries         maximal stretches of consecutive (finite) held samples
 *   plane 3   first_held      the first tick at which it holds
 *   plane 4   last_held       the last tick at which it holds
 *   plane 5   prefix_len      the stretch that begins at the first finite sample; 0: the first finite sample does not hold
 *   plane 6   prefix_end      its last tick
 *   plane 7   suffix_len      the stretch that ends at the last finite sample; 0: the last finite sample does not hold
 *   plane 8   suffix_start    its first tick
 *   plane 9   longest_len     the EARLIEST stretch of maximal length
 *   plane 10  longest_start   its first tick
 *   plane 11  longest_end     its last tick
 * The rule, for one finite sample (h, t) after the others: before = count, count++; if h: held++; if suffix_len == 0: entries++,
 * suffix_start = t; first_held = first_held ? first_held : t; last_held = t; suffix_len++; if prefix_len == before: prefix_len++,
 * prefix_end = t; if suffix_len > longest_len (strictly): longest = (suffix_len, suffix_start, t); otherwise suffix_len = 0,
 * suffix_start = 0.  And for two records, a earlier and b later (an empty side returns the other): the counts add; joined =
 * a.suffix_len > 0 && b.prefix_len > 0; entries = a.entries + b.entries - joined; first_held = a's or else b's; last_held = b's
 * or else a's; the prefix is a's unless a.prefix_len == a.count, then (a.count + b.prefix_len, b.prefix_len ? b.prefix_end :
 * a.prefix_end); the suffix is b's unless b.suffix_len == b.count, then (a.suffix_len + b.count, a.suffix_len ? a.suffix_start :
 * b.suffix_start); the longest is a's, then the joined stretch (a.suffix_len + b.prefix_len, a.suffix_start, b.prefix_end) if
 * joined and strictly longer, then b's if strictly longer.  All of it is integer, exact and associative in time order, and there
 * are no atomics, so every output is bit-identical however the range is cut into time segments (SIXDOF_DWELL_SEGMENTS in the
 * environment forces a count; 0 or unset: the library's choice), launches or calls.  Every word is below 2^53: a range whose last
 * sampled tick is 2^53 or more is refused.
 * SIXDOF_DWELL_HOLD, SIXDOF_DWELL_CONTINUE and SIXDOF_DWELL_ASYNC behave as SIXDOF_NORMS_HOLD, _CONTINUE and _ASYNC: the
 * accumulator is the call's staging buffer, and a continuing call is accepted only if the previous call succeeded with the same
 * conditions field for field (lo and hi compared by their bits) and the same period, ring bases, widths and row count are
 * unchanged, no sixdof_set_history or sixdof_bind_columns came since, and first_tick is above the last tick accumulated;
 * otherwise SIXDOF_ERR_INVALID_ARGUMENT and the accumulator stays as it was.
 * n_samples = 0 is a no-op that leaves the accumulator alone.  SIXDOF_ERR_INVALID_ARGUMENT, with nothing copied and the
 * accumulator as it was: everything sixdof_history_norms refuses (n_conditions in the place of n_probes, at most
 * SIXDOF_DWELL_MAX_CONDITIONS), an unknown kind or op, count != 1 with SIXDOF_DWELL_ELEMENT, a level that is not finite, hi != 0
 * with a one-sided op, lo > hi, a level below 0 with SIXDOF_DWELL_NORM_SQ.  A component the ring does not record:
 * SIXDOF_ERR_COMPONENT_NOT_FOUND.  A call that fails in the runtime leaves the ring as it was and the accumulator invalid, as for
 * sixdof_history_extremes. */
typedef struct sixdof_dwell_condition {   /* 64 bytes */
    sixdof_norm_probe probe;              /* as for sixdof_history_norms */
    double lo, hi;                        /* finite; SQUARED and >= 0 with SIXDOF_DWELL_NORM_SQ */
    uint32_t kind, op;                    /* SIXDOF_DWELL_ELEMENT or _NORM_SQ; SIXDOF_EVENT_LT .. _GE, SIXDOF_DWELL_INSIDE or _OUTSIDE */
} sixdof_dwell_condition;
#define SIXDOF_DWELL_ELEMENT 0u
#define SIXDOF_DWELL_NORM_SQ 1u
#define SIXDOF_DWELL_INSIDE  4u
#define SIXDOF_DWELL_OUTSIDE 5u
#define SIXDOF_DWELL_ASYNC    1u
#define SIXDOF_DWELL_CONTINUE 2u
#define SIXDOF_DWELL_HOLD     4u
#define SIXDOF_DWELL_PLANES   12
#define SIXDOF_DWELL_MAX_CONDITIONS 8
int sixdof_history_dwell(sixdof_handle* h, const sixdof_dwell_condition* conditions, size_t n_conditions, uint32_t period,
                         uint64_t first_tick, uint64_t n_samples, uint64_t every, double* host_dst, uint32_t flags);

/* ---- ring covariances: how quantities vary TOGETHER across the rows, over time ---------------------------------------------
 * The landing footprint ellipse, the 6 x 6 position / velocity dispersion, whether touchdown speed goes with lateral miss: joint
 * moments.  The envelope's mean and m2 are the diagonal of this matrix; the off-diagonals cannot be recovered from them.
 *
 * A channel is one element of one recorded component (the ones sixdof_history_read accepts; anything else:
 * SIXDOF_ERR_COMPONENT_NOT_FOUND); 2 <= n_channels = k <= SIXDOF_COVARIANCE_MAX_CHANNELS, from one component or several, a channel
 * may appear twice.  Samples and groups are sixdof_history_envelope's: for sample j (the state after tick first_tick + j * every)
 * and group g < period, the rows r with r % period == g are reduced jointly.  host_dst receives
 * [n_samples][period][1 + k + k (k + 1) / 2] doubles:
 *   count           rows used.  LISTWISE: a row is used only if all k channel values are finite, otherwise it is skipped for every
 *                   mean and every co-moment, so the matrix is that of one population (a non-finite value in an element that is
 *                   not listed skips nothing)
 *   mean[k]         over those rows
 *   C[a][b], a <= b row-major upper triangle of sum (x_a - mean_a)(x_b - mean_b) over them (covariance = C / count).
 * count = 0: everything behind the count is NaN.  Accumulated in f64 whatever the handle's dtype, by the multivariate Welford
 * update and Chan / Pebay merges, without FMA contraction.  No floating-point atomics; the launch geometry and merge order depend
 * on (n, period) only, so the values of one (tick, channel list, period) are bit-identical whichever range, `every` or flags read
 * them, and a channel listed twice gives C_aa, C_ab and C_bb bit-equal.
 * flags = 0: returns when the data is in host_dst.  SIXDOF_COVARIANCE_ASYNC: the rules of SIXDOF_WATCH_ASYNC — the copies go on
 * the copy stream, sixdof_download_wait blocks until they have landed, host_dst stays allocated (and page-locked) until
 * sixdof_sync.  Either way the ring is read on the compute stream: a later sixdof_step may overwrite the slots at once.
 * n_samples = 0 is a no-op.  SIXDOF_ERR_INVALID_ARGUMENT, with nothing copied: no ring, every = 0, period = 0, a row count that
 * is no multiple of period, period above 256 (the groups one block of the kernel keeps apart), n_channels outside 2 .. 6 (one
 * channel is the envelope's job), a null pointer, an element at or beyond its component's width, reserved != 0, a sampled tick
 * that is not (or no longer) in the ring, unknown flags.  A call that fails in the runtime leaves the ring as it was; a staging
 * or partial buffer that could not be grown is absent (size 0) and the next call allocates it again. */
typedef struct {
    uint64_t component_id;
    uint32_t element;  /* < the component's width */
    uint32_t reserved; /* 0 */
} sixdof_cov_channel;  /* 16 bytes */
#define SIXDOF_COVARIANCE_ASYNC 1u
#define SIXDOF_COVARIANCE_MAX_CHANNELS 6
int sixdof_history_covariance(sixdof_handle* h, const sixdof_cov_channel* channels, size_t n_channels, uint64_t first_tick,
                              uint64_t n_samples, uint64_t every, uint32_t period, double* host_dst, uint32_t flags);

/* ---- rollout models: systems piped AROUND six_dof, fused with it (the pipes of examples/<name>/sim.py) ------------- */
struct sixdof_apollo_tables; /* include/sixdof_apollo.h */
/* Select the Apollo-lander rollout model (examples/apollo-lander/sim.py:517-526 + the guidance sidecar
 * controller/src/main.rs).  Needs, besides the Body columns, the columns "apollo_state" [n,16],
 * "apollo_params" [n,17], "apollo_guidance" [n,8], "apollo_score" [n,4], "apollo_result" [n,12] bound
 * with sixdof_bind_columns; integrator must be SEMI_IMPLICIT, dtype F64.  Tables are copied. */
int sixdof_set_model_apollo(sixdof_handle* h, const struct sixdof_apollo_tables* tables);
/* D2H of any bound column by id (model columns are not covered by the sixdof_download mask). */
int sixdof_download_column(sixdof_handle* h, uint64_t component_id);
/* H2D of ONE bound column from its host buffer: how an external write to a component (StepContext.write_component,
 * libs/nox-py/src/step_context.rs; copy_db_to_world's per-component copy, impeller2_server.rs:320-362) reaches the device between
 * batches without re-uploading the columns the host never downloaded.  Needs a prior sixdof_upload. */
int sixdof_upload_column(sixdof_handle* h, uint64_t component_id);

/* ---- campaign collectives: Monte-Carlo rollouts sharded over the GPUs of one node ---------------------------------------
 * The reference runs one OS process per rollout with nothing exchanged between them (libs/monte-carlo/src/lib.rs:2083): the
 * plan row reaches a run through its context file and result.json comes back through the file system.  With rollouts as
 * column rows on several GPUs the two movements are ONE broadcast of the plan table from rank 0 and ONE gather of the
 * result rows, in run-id order (row = idx, run_id = run_%07d, seed = idx + 1: sample.py:149) — RCCL over xGMI, loaded
 * with dlopen (a single-GPU host never needs it).  No exchange per step.  One communicator = one rank = one GPU = one
 * caller thread, like a handle.  The 128-byte id is RCCL's ncclUniqueId: rank 0 makes it, the host ships it to the other
 * ranks by whatever channel it already has (the runner's job file, an env var, a socket). */
typedef struct sixdof_comm sixdof_comm;
#define SIXDOF_COMM_ID_BYTES 128
int sixdof_comm_unique_id(uint8_t id[SIXDOF_COMM_ID_BYTES]);                       /* SIXDOF_ERR_UNSUPPORTED: no RCCL here */
int sixdof_comm_init(sixdof_comm** out, const uint8_t id[SIXDOF_COMM_ID_BYTES], int world, int rank, int device_ordinal);
void sixdof_comm_destroy(sixdof_comm* c);
const char* sixdof_comm_last_error(const sixdof_comm* c);                          /* c may be NULL: last init error */
/* Rank r's contiguous block [lo, hi) of n_rows run ids (blocks differ by at most one row). */
void sixdof_shard_range(uint64_t n_rows, int world, int rank, uint64_t* lo, uint64_t* hi);
/* The gather's packing without a transport (pure host code): equal blocks of sixdof_gather_block_rows(n_total, world) =
 * ceil(n_total / world) rows, rank r's rows first and zeros after; `blocks` = the `world` blocks in rank order.  What
 * sixdof_campaign_gather runs around its one ncclAllGather, and what a host with its own transport runs around its. */
uint64_t sixdof_gather_block_rows(uint64_t n_total, int world);
int sixdof_gather_pack(const double* local_rows, uint64_t n_local, uint64_t width, uint64_t n_total, int world, int rank, double* block);
int sixdof_gather_unpack(const double* blocks, uint64_t width, uint64_t n_total, int world, double* all_rows);
/* `root`'s host buffer of n_bytes (the plan table [n_runs, n_params] f64, a reference profile ...) -> every rank's. */
int sixdof_campaign_broadcast(sixdof_comm* c, void* table, uint64_t n_bytes, int root);
/* Every rank contributes its block's result rows [n_local, width] f64 (n_local = its sixdof_shard_range of n_total);
 * every rank receives all [n_total, width] rows in run-id order. */
int sixdof_campaign_gather(sixdof_comm* c, const double* local_rows, uint64_t n_local, uint64_t width, double* all_rows,
                           uint64_t n_total);

#ifdef __cplusplus
}
#endif
#endif /* SIXDOF_HIP_H */
