// step_plan.hpp — how sixdof_step splits a batch of ticks into launches, and which of them replay.  Pure host code, no HIP:
// the step kernel's AQL, hipGraph and eager paths (sixdof_capi.cpp) run batches by plan_batch; aql_packet_test.cpp checks it.
#pragma once

#include <cstdint>

namespace sixdof {

// Launches per replayed chain.  A long chain amortises the gap between two replays (4,096 launches: 4.96 -> 4.83 us each with
// 128-launch chains) but starts later (100 launches as one chain: 8 % slower than 32 + 32 + 32 + 4), so a batch OPENS with a
// 32-launch chain and, when at least four fit, continues with 128-launch ones (profiles/r02_graph_len_ab.txt).
constexpr uint32_t kGraphLen = 32;
constexpr uint32_t kGraphLong = 128;
constexpr uint32_t kGraphMinLen = 4;   // shorter chains are launched eagerly (a replay costs ~10-16 us of host time)

// What a batch of `full` K-tick launches replays, in this order: an opening 32-launch chain (long batches only: 200
// launches as 32 + 128 + 40 measured 5 % slower), `n_long` 128-launch chains, `n_short` further 32-launch chains, and one
// chain of the `tail` launches left (0 when fewer than kGraphMinLen: those run eagerly).  A short batch as a whole, e.g.
// 20 launches, is its tail — so a short timed region is steady-state device work too, not eager launches racing the host.
struct ChainPlan {
    bool open = false;
    uint64_t n_long = 0, n_short = 0;
    uint32_t tail = 0;
    uint64_t launches() const { return (open ? kGraphLen : 0) + n_long * kGraphLong + n_short * kGraphLen + tail; }
};

inline ChainPlan plan_chains(uint64_t full) {
    ChainPlan c;
    if (full >= kGraphLen + 4 * kGraphLong) {
        c.open = true;
        c.n_long = (full - kGraphLen) / kGraphLong;
        full -= kGraphLen + c.n_long * kGraphLong;
    }
    c.n_short = full / kGraphLen;
    if (full % kGraphLen >= kGraphMinLen) c.tail = static_cast<uint32_t>(full % kGraphLen);
    return c;
}

// The launches of a batch, in order: the accel-check launch of `check_ticks` ticks (0: none), `full` K-tick launches, and
// one launch of the `rem` ticks left (0: none).  The check launch is one of the K-tick launches, or the whole batch when
// that is shorter than K.  `chains`: how many of the `full` launches replay; the rest run eagerly.
struct BatchPlan {
    uint32_t check_ticks = 0;
    uint64_t full = 0;
    uint32_t rem = 0;
    ChainPlan chains;
    uint64_t launches() const { return (check_ticks ? 1 : 0) + full + (rem ? 1 : 0); }
};

// `check`: the batch opens with the accel-check launch.  `replay`: the handle replays chains (else `chains` stays empty).
inline BatchPlan plan_batch(uint64_t n_ticks, uint32_t K, bool check, bool replay) {
    BatchPlan b;
    b.full = n_ticks / K;
    b.rem = static_cast<uint32_t>(n_ticks % K);
    if (check && n_ticks > 0) {
        b.check_ticks = static_cast<uint32_t>(n_ticks < K ? n_ticks : K);
        if (b.full) b.full -= 1;
        else b.rem = 0;
    }
    if (replay) b.chains = plan_chains(b.full);
    return b;
}

}  // namespace sixdof
