// history_plan_test.cpp — host unit test of history_plan.hpp: the validity rule of a sampled range at its edges, and the
// slot sequence of wrapping, strided ranges against a brute-force twin that simulates the ring slot by slot, and the rule at
// every = 1 against the hand-written predicate sixdof_history_read / sixdof_history_stream used to carry.  No GPU.
// Prints "history plan test ok" on success (tests/test_history_plan.py).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "history_plan.hpp"

using namespace sixdof;

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                     \
        }                                                                     \
    } while (0)

namespace {

// The ring as the recorder fills it: tick t = 1, 2, ... goes to the slot after the previous one, starting at slot 0, and
// wraps.  holds[s] is the tick slot s holds after `tick` ticks (0: never written or recorded before `hist_first_tick`).
std::vector<uint64_t> simulate_ring(uint64_t hist_first_tick, uint64_t tick, uint64_t ring) {
    std::vector<uint64_t> holds(ring, 0);
    uint64_t slot = 0;
    for (uint64_t t = 1; t <= tick; t++) {
        if (t >= hist_first_tick) holds[slot] = t;
        slot = slot + 1 == ring ? 0 : slot + 1;
    }
    return holds;
}

// Brute force: every sampled tick is found in the simulated ring.
bool brute_ok(uint64_t first_tick, uint64_t n_samples, uint64_t every, const std::vector<uint64_t>& holds) {
    if (every == 0 || n_samples == 0) return false;
    for (uint64_t j = 0; j < n_samples; j++) {
        const uint64_t want = first_tick + j * every;
        bool found = false;
        for (uint64_t held : holds) found |= held != 0 && held == want;
        if (!found) return false;
    }
    return true;
}

void test_rule_edges() {
    // ring of 10, recording since tick 6, 30 ticks done: ticks 21 .. 30 are in the ring
    const uint64_t hf = 6, tick = 30, ring = 10;
    CHECK(sampled_range_ok(21, 10, 1, hf, tick, ring));
    CHECK(sampled_range_ok(21, 1, 1, hf, tick, ring));
    CHECK(sampled_range_ok(30, 1, 1, hf, tick, ring));
    CHECK(sampled_range_ok(30, 1, 1000, hf, tick, ring));     // one sample: the stride does not matter
    CHECK(!sampled_range_ok(20, 1, 1, hf, tick, ring));       // fallen out of the ring
    CHECK(!sampled_range_ok(31, 1, 1, hf, tick, ring));       // not computed yet
    CHECK(!sampled_range_ok(21, 11, 1, hf, tick, ring));      // runs past `tick`
    CHECK(sampled_range_ok(21, 4, 3, hf, tick, ring));        // 21 24 27 30
    CHECK(!sampled_range_ok(21, 5, 3, hf, tick, ring));       // ... 33
    CHECK(sampled_range_ok(22, 3, 3, hf, tick, ring));        // 22 25 28
    CHECK(!sampled_range_ok(22, 4, 3, hf, tick, ring));       // ... 31
    CHECK(!sampled_range_ok(21, 1, 0, hf, tick, ring));       // every = 0
    CHECK(!sampled_range_ok(21, 0, 1, hf, tick, ring));       // the caller treats 0 samples as a no-op before asking
    CHECK(!sampled_range_ok(21, 1, 1, hf, tick, 0));          // no ring
    CHECK(!sampled_range_ok(0, 1, 1, 0, tick, 64));           // tick 0 is the spawned state: never recorded
    // the ring has not wrapped yet: the first recorded tick bounds the range
    CHECK(sampled_range_ok(6, 3, 1, 6, 8, 10));
    CHECK(!sampled_range_ok(5, 1, 1, 6, 8, 10));
    CHECK(!sampled_range_ok(9, 1, 1, 6, 8, 10));
    // nothing recorded since the ring was enabled
    CHECK(!sampled_range_ok(31, 1, 1, 31, 30, 10));
    // no overflow near the top of the range
    const uint64_t top = UINT64_MAX;
    CHECK(sampled_range_ok(top - 4, 2, 3, 1, top - 1, 8));    // top-4, top-1
    CHECK(!sampled_range_ok(top - 4, 3, 3, 1, top - 1, 8));   // the third sample would wrap 64 bits
    CHECK(!sampled_range_ok(top - 4, top, top, 1, top - 1, 8));
    CHECK(!sampled_range_ok(2, 2, top, 1, top - 1, top));
}

void test_against_brute_force() {
    uint64_t checked = 0, valid = 0;
    for (uint64_t ring : {1, 2, 3, 7, 8, 10}) {
        for (uint64_t hf : {1, 4, 9}) {
            for (uint64_t tick : {0, 3, 8, 9, 10, 11, 27, 40}) {
                const std::vector<uint64_t> holds = simulate_ring(hf, tick, ring);
                for (uint64_t first = 0; first <= tick + 2; first++) {
                    for (uint64_t every : {0, 1, 2, 3, 7, 11}) {
                        for (uint64_t ns = 0; ns <= ring + 2; ns++) {
                            const bool ok = sampled_range_ok(first, ns, every, hf, tick, ring);
                            CHECK(ok == brute_ok(first, ns, every, holds));
                            checked++;
                            if (!ok) continue;
                            valid++;
                            // the slot function finds each sampled tick where the recorder left it
                            for (uint64_t j = 0; j < ns; j++) {
                                const uint64_t s = sample_slot(first, j, every, ring);
                                CHECK(s < ring);
                                CHECK(holds[s] == first + j * every);
                            }
                        }
                    }
                }
            }
        }
    }
    CHECK(checked > 10000 && valid > 500);
}

// What sixdof_history_stream (and, with n_ticks = 1, sixdof_history_read) checked by hand before they took the shared rule:
// the specification the rule is held to at every = 1.  In 64 bits, wrap included, as that code computed it.
bool contiguous_run_ok(uint64_t first_tick, uint64_t n_ticks, uint64_t hist_first_tick, uint64_t tick, uint64_t ring) {
    const uint64_t last = first_tick + n_ticks - 1;
    return !(first_tick < hist_first_tick || last > tick || first_tick + ring <= tick || n_ticks > ring);
}

void test_contiguous_runs_classified_as_before() {
    uint64_t valid = 0;
    for (uint64_t ring = 1; ring <= 5; ring++)
        for (uint64_t hf = 1; hf <= 4; hf++)
            for (uint64_t tick = 0; tick <= 9; tick++)
                for (uint64_t first = 0; first <= 11; first++)
                    for (uint64_t n = 1; n <= 7; n++) {
                        const bool ok = sampled_range_ok(first, n, 1, hf, tick, ring);
                        CHECK(ok == contiguous_run_ok(first, n, hf, tick, ring));
                        valid += ok;
                    }
    CHECK(valid > 100);
    // where only the hand-written form could wrap (first_tick + n_ticks - 1 == 0): it refused through n_ticks > ring
    const uint64_t top = UINT64_MAX;
    for (uint64_t ring : {uint64_t(1), uint64_t(4), uint64_t(1) << 32})
        for (uint64_t tick : {uint64_t(2), uint64_t(5), top - 1}) {
            CHECK(!contiguous_run_ok(2, top, 1, tick, ring));
            CHECK(!sampled_range_ok(2, top, 1, 1, tick, ring));
        }
}

void test_wrapping_strided_sequence() {
    // ring 10, ticks 18 .. 27 wrap: slots 7 8 9 0 1 .. 6
    const uint64_t want1[10] = {7, 8, 9, 0, 1, 2, 3, 4, 5, 6};
    for (uint64_t j = 0; j < 10; j++) CHECK(sample_slot(18, j, 1, 10) == want1[j]);
    // every third of them: ticks 18 21 24 27
    const uint64_t want3[4] = {7, 0, 3, 6};
    for (uint64_t j = 0; j < 4; j++) CHECK(sample_slot(18, j, 3, 10) == want3[j]);
    // a stride that does not divide the ring: ring 64, ticks 1 8 15 .. 50
    for (uint64_t j = 0; j < 8; j++) CHECK(sample_slot(1, j, 7, 64) == 7 * j);
    CHECK(history_slot(1, 64) == 0 && history_slot(64, 64) == 63 && history_slot(65, 64) == 0);
    // slot * n * w needs 64 bits at the workload's sizes: the slot itself stays exact beyond 2^32 ticks
    CHECK(history_slot((uint64_t(1) << 40) + 5, 1000) == ((uint64_t(1) << 40) + 4) % 1000);
}

}  // namespace

int main() {
    test_rule_edges();
    test_against_brute_force();
    test_contiguous_runs_classified_as_before();
    test_wrapping_strided_sequence();
    std::printf("history plan test ok\n");
    return 0;
}
