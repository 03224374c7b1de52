// kernels.hpp — launch interface between the C-ABI host layer (sixdof_capi.cpp) and the gfx950
// kernels (sixdof_kernels.hip, nbody_kernels.hip).  Internal; not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Floating-point contraction is decided per SOURCE EXPRESSION (a * b + c written as one expression becomes one FMA) and
// nowhere else.  hipcc's default for device code ("fast") also fuses a multiply and an add that merely end up in the
// same basic block after inlining — so two inlined copies of the same tick body (loop body vs last tick, one launch
// shape vs another) could round differently.  With "on" every instantiation of the kernels computes the same bits:
// results do not depend on ticks_per_launch, graph replay, cache policy or which copy of the body ran a tick
// (tests/test_gpu_parity.py::test_fused_ticks_match_single_tick_launches).  Applies to everything that includes this
// header, generated translation units included.
#pragma clang fp contract(on)

namespace sixdof {

constexpr int kMaxOps = 4;       // per-entity effector ops fused into the step kernel
constexpr int kMaxModelCols = 128; // component columns of a generated program (kernarg: 2 pointers each; 128 keep StepParams at 2.4 KB of the 4 KB limit)
constexpr int kBlock = 256;      // threads per workgroup = entities per workgroup (4 waves of 64)

// One effector op as the kernel sees it (sixdof_effector_op with the aux column resolved).
struct DevOp {
    int32_t kind;
    int32_t aux_width;  // row width of `aux` (1..3); 0 = 3
    const void* aux;    // device [n,aux_width] column (element type = state dtype) or nullptr
    double p[6];
};

// Kernel argument block of the fused per-entity step.  Columns are device pointers in the
// reference's row-major layout: pos [n,7], vel [n,6], accel [n,6], force [n,6], inertia [n,7].
struct StepParams {
    void* pos;
    void* vel;
    void* accel;
    void* force;
    const void* inertia;
    uint32_t n;
    uint32_t n_ticks;         // ticks fused into this launch
    double dt_g;              // globals simulation_time_step (RK4 stage offsets)
    double dt;                // six_dof(time_step=) override or dt_g (final combination / semi-implicit)
    uint32_t n_ops;
    uint32_t vel_independent; // 1: no op reads the stage velocity -> RK4 stages 1 and 2 share F and A
    uint32_t streaming;       // cache-policy code of the launch: load policy * 8 + store policy (step_kernel.hpp)
    uint32_t hist_ring;       // history ring length in ticks (0 = off)
    uint64_t hist_slot0;      // ring slot index (before modulo) of the first tick of this launch
    void* hist_pos;           // [ring][n,7]   per-tick outputs, reference row layout; nullptr = no recording
    void* hist_vel;           // [ring][n,6]
    void* hist_accel;         // [ring][n,6]
    void* hist_force;         // [ring][n,6]
    uint64_t tick0;           // tick count before this launch (generated systems may read the tick)
    uint32_t accel_in_check;  // 1: the world_accel column holds HOST data (first launch after an upload): RK4 stage 0 reads it
                              //    the way the reference does, v_s = v0 + 0 * a_in (rk4.rs:96-100), so a non-finite row poisons the tick
    uint32_t state_only;      // 1: store world_pos / world_vel only.  For a launch of a batch that another launch follows inside the same
                              //    sixdof_step call: nothing reads world_accel / force before that launch overwrites them.  Built-in pipes
                              //    only, never with the history ring or accel_in_check (sixdof_capi.cpp state_only_eligible)
    DevOp ops[kMaxOps];
    // generated programs only — behind everything the hand-written kernels read, so their kernarg loads stay within the
    // first 400 bytes whatever kMaxModelCols is
    void* model_cols[kMaxModelCols];  // device [n,w] component columns, read and written
    void* model_hist[kMaxModelCols];  // their history rings [ring][n,w] (nullptr = not recorded)
};

enum : int { kRk4 = 0, kSemiImplicit = 1, kNone = 2 };   // kNone: a pipe of systems without six_dof (generated programs only)

// One launch of the built-in step kernel: the instantiation's host stub (null: nothing to launch) and its grid of
// kWave-thread workgroups.
struct StepKernel {
    const void* fn = nullptr;
    dim3 grid;
};

// The instantiation launch_step runs for `p` (built-in pipes only).
StepKernel select_step(const StepParams& p, int integrator, int dtype);

// Fused clear_forces | effectors | calc_accel | integrator over n entities, n_ticks ticks.
// dtype: 0 = f64, 1 = f32.  Returns the launch's error.
hipError_t launch_step(const StepParams& p, int integrator, int dtype, hipStream_t stream);

// Entry points of a run-time generated effector pipe (elodin_amd/codegen.py), resolved with dlsym.
using CustomAbiFn = unsigned (*)();                                               // sizeof(StepParams) it was built with
using CustomLayoutFn = unsigned (*)();                                            // n_aux | n_model_cols << 8 | writes_inertia << 16
using CustomLaunchFn = int (*)(const StepParams*, int integrator, int dtype, void* stream);  // returns hipError_t

// ---- pairwise (edge_fold) path -----------------------------------------------------------------------
// Kernels and launch templates: pair_kernel.hpp (built-in folds: nbody_kernels.hip; user-written folds: generated units).
// A batch of ticks is one pack launch, then per tick: all-pairs = accumulate + integrate (2 launches); edge lists = ONE
// fold-and-integrate launch (+ 2 hub launches when there are hub sources); n <= kPairSmallMax = one launch for the whole batch.
// Every tick writes the next tick's pack rows.
constexpr int kPackWidth = 10;   // per source: p(c=0) p(c=1/2) p(c=1) mass
constexpr int kPartialForce = 9;  // all-pairs gravity writes forces only
constexpr int kPartialWidth = 18; // per target and source split: 3 stage positions x Force [tau(3), f(3)]

struct PairParams {
    void* pos;            // [n,7]
    void* vel;            // [n,6]
    void* accel;          // [n,6]
    void* force;          // [n,6]
    const void* inertia;  // [n,7]
    uint32_t n;
    double dt_g, dt;
    double* pack;         // [n,10] scratch
    double* pack_next;    // [n,10] the pack rows the one-launch sparse tick writes for the NEXT tick (pair_kernel.hpp 3b); nullptr: not provided
    double* partial;      // [splits,n,partial_width] scratch
    uint32_t splits;      // source-range splits of the all-pairs kernel (1 for edge lists)
    uint32_t partial_width;  // kPartialForce (all-pairs: 3 stages x force) or kPartialWidth (3 stages x [tau, f])
    // edge list in CSR-by-source form (spawn order preserved inside a source), device
    const uint32_t* row_start;  // [n+1]
    const uint32_t* dst;        // [n_edges]
    uint32_t n_edges;
    // hub sources (out-degree >= kHubDegree), folded by whole waves instead of one lane each (pair_kernel.hpp 2c):
    // their edge ranges cut into chunks of <= kHubChunk edges
    uint32_t n_hubs, n_hub_chunks;
    const uint32_t* hub_rows;          // [n_hubs] source rows
    const uint32_t* hub_chunk_start;   // [n_hubs+1] first chunk of each hub
    const uint32_t* chunk_e0;          // [n_hub_chunks] first edge of each chunk (it ends kHubChunk later or with its source)
    const uint32_t* chunk_row;         // [n_hub_chunks] the chunk's source row
    double* chunk_partial;             // [n_hub_chunks, kPartialWidth] scratch
    int32_t pair_kind;    // sixdof_effector_kind 6,7,8
    double p0, p1;        // G | K, eps
    uint32_t n_ops;       // per-entity ops applied BEFORE the pair op (pipe order); they survive only on
    DevOp ops[kMaxOps];   // rows that are not edge sources (edge_fold replaces Force on source rows)
    // 1: `pack` already holds the rows of the current state (the previous tick's integrate kernel wrote them, and nothing has
    // touched pos / vel / inertia since): the batch starts without a pack launch.  Set by the caller inside ONE step call only —
    // between calls a host may write the columns (upload, sixdof_device_column), so every call packs once.
    uint32_t packed;
};
// Picks the number of source splits for n targets so the all-pairs grid fills 256 CUs.
uint32_t pair_splits_for(uint32_t n);
// n_ticks ticks: one pack launch (all-pairs: unless p.packed), then the tick's launches as above.  An edge list needs p.pack_next.
hipError_t launch_pair_ticks(const PairParams& p, int integrator, uint32_t n_ticks, hipStream_t stream, uint64_t* launches);
// n <= kPairSmallMax: pack, fold and integrate n_ticks ticks in one single-workgroup launch (bit-identical results).
constexpr uint32_t kPairSmallMax = 256;
constexpr uint32_t kHubDegree = 32;    // a source with this many out-edges or more is a hub
constexpr uint32_t kHubChunk = 256;    // edges one wave folds (4 per lane: a short dependent-gather chain)
hipError_t launch_pair_small(const PairParams& p, int integrator, uint32_t n_ticks, hipStream_t stream,
                             uint64_t* launches);
// Entry points of a generated pair-fold translation unit (codegen.py: generate_pair_source).
using CustomPairAbiFn = unsigned (*)();
using CustomPairLaunchFn = int (*)(const PairParams* p, int integrator, uint32_t n_ticks, int small, void* stream,
                                   uint64_t* launches);

// ---- joins (query.rs:599-725): gather / scatter of rows by constant u32 indices -----------------------------
hipError_t launch_gather_rows(void* dst, const void* src, const uint32_t* rows, uint32_t m, uint32_t w, size_t elem,
                              hipStream_t s);
hipError_t launch_scatter_rows(void* dst, const void* src, const uint32_t* rows, uint32_t m, uint32_t w, size_t elem,
                               hipStream_t s);

// ---- watch lists: dense time series of chosen rows gathered out of the telemetry ring (join_kernels.hip) -----
constexpr uint32_t kHistoryGatherMax = 32;   // components one launch covers (blockIdx.y)
struct HistoryGatherDesc {
    const void* ring;      // [ring][n, w] blocks of this component
    uint64_t out_offset;   // where its [m][n_samples][w] block starts in `out`, in elements
    uint32_t w;
    uint32_t reserved;
};
struct HistoryGatherArgs { HistoryGatherDesc c[kHistoryGatherMax]; };   // by value: 768 bytes of kernel arguments
// Sample j of row rows[e] = tick first_tick + j * every, for e < m, j < n_samples; the caller has validated the range
// (history_plan.hpp: sampled_range_ok) and rows[e] < n.
hipError_t launch_history_gather(const HistoryGatherArgs& a, uint32_t n_components, void* out, const uint32_t* rows,
                                 uint64_t m, uint64_t n, uint64_t first_tick, uint64_t n_samples, uint64_t every,
                                 uint64_t ring, size_t elem, hipStream_t s);

// ---- ring reductions: one sampled tick of one component reduced into period * w (group, element) bins ---------------------
// One component of a launch, for every kernel that reduces into bins (envelope_kernels.hip, quantile_kernels.hip): blockIdx.z
// picks it.  sixdof_capi.cpp's ring_bin_read fills these.
constexpr uint32_t kRingBinMaxComponents = 32;   // components one launch covers
struct RingBinDesc {
    const void* ring;         // [ring][n, w] blocks of this component
    uint64_t out_offset;      // where its [n_samples][period][planes][w] block starts in `out`, in doubles
    uint64_t scratch_offset;  // where its units of one sample start in a sample's scratch, in the reduction's own units
    uint32_t w;
    uint32_t reserved;
};
struct RingBinArgs { RingBinDesc c[kRingBinMaxComponents]; };   // by value: 1 KiB of kernel arguments

// ---- ring envelopes: count / min / max / mean / m2 across the rows of every sampled tick (envelope_kernels.hip) -----
// 5 planes; a scratch unit is one EnvelopePartial record, [blocks][period * w] of them per component and sample.
// Samples sample0 .. sample0 + n_samples - 1 (n_samples < 65,536) of the range first_tick, first_tick + every, ...: stage 1 writes
// `partial_stride` records (envelope_plan.hpp: EnvelopePartial) per sample into `partial`, stage 2 merges them in index order into
// `out`.  The caller has validated the range (sampled_range_ok), n % period == 0 and envelope_supported(w, period).
hipError_t launch_history_envelope(const RingBinArgs& a, uint32_t n_components, double* out, void* partial, uint64_t partial_stride,
                                   uint64_t n, uint32_t period, uint64_t first_tick, uint64_t sample0, uint64_t n_samples,
                                   uint64_t every, uint64_t ring, size_t elem, hipStream_t s);

// ---- ring quantiles: exact order statistics across the rows of every sampled tick (quantile_kernels.hip) ------------------
// 1 + 2 * ranks planes; a scratch unit is one (bin, rank) slot, period * w * ranks of them per component and sample.
struct QuantileRanks;   // quantile_plan.hpp
// Samples sample0 .. sample0 + n_samples - 1 (n_samples < 65,536) of the range first_tick, first_tick + every, ...  Per sample
// `slot_stride` (bin, rank) slots: `hist` holds 256 uint32 counters per slot, `state` one QuantileSlot (quantile_plan.hpp); both
// are scratch the launches clear themselves.  The caller has validated the range (sampled_range_ok), the ranks, n % period == 0
// and envelope_supported(w, period).
hipError_t launch_history_quantiles(const RingBinArgs& a, uint32_t n_components, const QuantileRanks& ranks, double* out, void* hist,
                                    void* state, uint64_t slot_stride, uint64_t n, uint32_t period, uint64_t first_tick,
                                    uint64_t sample0, uint64_t n_samples, uint64_t every, uint64_t ring, size_t elem, hipStream_t s);

// ---- ring extremes: per row and element, min / max over the sampled ticks and the ticks they fall on (extremes_kernels.hip) ---
// 6 planes; here a component's block in `out` is [6][n * w] doubles at out_offset, and a scratch unit is one element: its records
// start at scratch_offset in every segment's `scratch_stride` units.  All n_samples samples of the range first_tick, first_tick +
// every, ... in `segments` time segments (extremes_plan.hpp); with more than one, `scratch` holds segments * 6 * scratch_stride
// 64-bit words.  merge_into: `out` holds the planes of the samples before this range, and the result covers both.  The caller has
// validated the range (sampled_range_ok, scan_ticks_ok).
hipError_t launch_history_extremes(const RingBinArgs& a, uint32_t n_components, double* out, void* scratch, uint64_t scratch_stride,
                                   uint32_t segments, bool merge_into, uint64_t n, uint64_t first_tick, uint64_t n_samples, uint64_t every,
                                   uint64_t ring, size_t elem, hipStream_t s);

// ---- ring events: per trigger and run, the first threshold crossing over the sampled ticks and the state there (events_kernels.hip) ---
struct EventsArgs;   // events_plan.hpp: the triggers (ring base, width, element, group, op, mode, level) of one launch, at most 8
// All n_samples samples of the range first_tick, first_tick + every, ... in `segments` time segments (events_plan.hpp).  `rec`:
// the records, [n_triggers][10][runs] 64-bit words with runs = n / period, written by every launch and read first when merge_into
// (they then hold the samples before this range, and the result covers both); `out`: the four planes, [n_triggers][4][runs]
// doubles; with more than one segment `scratch` holds segments * n_triggers * 10 * runs words.  The caller has validated the range
// (sampled_range_ok, scan_ticks_ok) and the triggers (events_launch_ok).
hipError_t launch_history_events(const EventsArgs& a, uint32_t n_triggers, void* rec, double* out, void* scratch, uint32_t segments, bool merge_into,
                                 uint64_t n, uint32_t period, uint64_t first_tick, uint64_t n_samples, uint64_t every, uint64_t ring, size_t elem,
                                 hipStream_t s);
// After it, on the same stream: for at most kRingBinMaxComponents captured components (c: ring, width and out_offset, where the
// component's [n_triggers][n * w] doubles start in `out`), the ring's elements at the tick `rec` reports for the element's run,
// where that tick is one of this range's samples; elsewhere NaN, or (merge_into) what `out` held.
hipError_t launch_events_capture(const EventsArgs& a, uint32_t n_triggers, const RingBinArgs& c, uint32_t n_captures, const void* rec, double* out,
                                 bool merge_into, uint64_t n, uint32_t period, uint64_t first_tick, uint64_t n_samples, uint64_t every, uint64_t ring,
                                 size_t elem, hipStream_t s);

// ---- ring norms: per probe and run, the extremes of a squared vector length or separation over the sampled ticks (norms_kernels.hip) ---
struct NormsArgs;   // norms_plan.hpp: the probes (ring bases, widths, elements, groups, count, flags) of one launch, at most 8
// All n_samples samples of the range first_tick, first_tick + every, ... in `segments` time segments (norms_plan.hpp).  `out`: the
// six planes, [n_probes][6][runs] doubles with runs = n / period, read first when merge_into (they then hold the samples before
// this range, and the result covers both); with more than one segment `scratch` holds segments * n_probes * 6 * runs 64-bit words.
// The caller has validated the range (sampled_range_ok, scan_ticks_ok) and the probes (norms_launch_ok).
hipError_t launch_history_norms(const NormsArgs& a, uint32_t n_probes, double* out, void* scratch, uint32_t segments, bool merge_into, uint64_t n,
                                uint32_t period, uint64_t first_tick, uint64_t n_samples, uint64_t every, uint64_t ring, size_t elem, hipStream_t s);

// ---- ring norm events: per trigger and run, the first crossing of a squared vector length or separation and the state there (norm_events_kernels.hip) ---
struct NormEventsArgs;   // norm_events_plan.hpp: the triggers (a norms probe, level_sq, op, mode) of one launch, at most 8
// All n_samples samples of the range first_tick, first_tick + every, ... in `segments` time segments (norm_events_plan.hpp).  `rec`,
// `out` and `scratch` as for launch_history_events — the records have the events' layout, so launch_events_capture follows on the
// same stream with norm_events_capture_args.  The caller has validated the range (sampled_range_ok, scan_ticks_ok) and the
// triggers (norm_events_launch_ok).
hipError_t launch_history_norm_events(const NormEventsArgs& a, uint32_t n_triggers, void* rec, double* out, void* scratch, uint32_t segments, bool merge_into,
                                      uint64_t n, uint32_t period, uint64_t first_tick, uint64_t n_samples, uint64_t every, uint64_t ring, size_t elem,
                                      hipStream_t s);

// ---- ring dwell: per condition and run, how long and how often a predicate held over the sampled ticks (dwell_kernels.hip) ---
struct DwellArgs;   // dwell_plan.hpp: the conditions (a norms probe, kind, op, lo, hi) of one launch, at most 8
// All n_samples samples of the range first_tick, first_tick + every, ... in `segments` time segments (dwell_plan.hpp).  `out`: the
// twelve planes, [n_conditions][12][runs] doubles with runs = n / period, read first when merge_into (they then hold the samples
// before this range, and the result covers both); with more than one segment `scratch` holds segments * n_conditions * 12 * runs
// 64-bit words.  The caller has validated the range (sampled_range_ok, scan_ticks_ok) and the conditions (dwell_launch_ok).
hipError_t launch_history_dwell(const DwellArgs& a, uint32_t n_conditions, double* out, void* scratch, uint32_t segments, bool merge_into, uint64_t n,
                                uint32_t period, uint64_t first_tick, uint64_t n_samples, uint64_t every, uint64_t ring, size_t elem, hipStream_t s);

// ---- ring covariances: count, mean vector and co-moment matrix of k channels across the rows of every sampled tick (covariance_kernels.hip) ---
constexpr uint32_t kCovarianceArgChannels = 6;   // covariance_plan.hpp: kCovarianceMaxChannels
struct CovarianceChannel {
    const void* ring;   // [ring][n, w] blocks of the channel's component
    uint32_t w;
    uint32_t element;   // < w
};
struct CovarianceArgs { CovarianceChannel c[kCovarianceArgChannels]; };   // by value: 96 bytes of kernel arguments
// Samples sample0 .. sample0 + n_samples - 1 (n_samples < 65,536) of the range first_tick, first_tick + every, ...: stage 1 writes
// `partial_stride` doubles per sample into `partial` (covariance_plan.hpp: covariance_scratch_doubles), stage 2 merges them in
// block order into `out`, [n_samples of the whole read][period][1 + k + k (k + 1) / 2] doubles.  The caller has validated the range
// (sampled_range_ok), n % period == 0, covariance_supported(k, period) and every element < w.
hipError_t launch_history_covariance(const CovarianceArgs& a, uint32_t k, double* out, void* partial, uint64_t partial_stride, uint64_t n, uint32_t period,
                                     uint64_t first_tick, uint64_t sample0, uint64_t n_samples, uint64_t every, uint64_t ring, size_t elem, hipStream_t s);

hipError_t launch_nonfinite(const void* pos, const void* vel, uint32_t n, size_t elem, uint8_t* flags,
                            unsigned long long* count, hipStream_t s);

// ---- Apollo-lander rollout model (include/sixdof_apollo.h) ---------------------------------------------
struct ApolloParams {
    double *pos, *vel, *accel, *force, *inertia;  // Body columns
    double* state;           // [n,16]
    const double* params;    // [n,17]
    double* guidance;        // [n,8]
    double* score;           // [n,4]
    double* result;          // [n,12]
    const double* tick_refs; // [n_ticks,8] per-tick reference profile values, device
    uint32_t n;
    uint32_t n_ticks;
    uint64_t tick0;          // tick count before this launch
    uint64_t max_ticks;
    uint32_t guidance_period;
    uint32_t ticks_per_telemetry;  // post_step runs when a batch of this many ticks has completed (impeller2_server.rs:553-678)
    double dt;               // globals simulation_time_step
};
hipError_t launch_apollo(const ApolloParams& p, hipStream_t stream);

}  // namespace sixdof
