// aql_packet_test.cpp — host unit test of the AQL packet builder (aql_packets.cpp): header bits, fence scopes by
// position, grid in work-items, segment sizes, argument-block address, ring wrap-around and flow control.  No GPU, no
// HSA runtime: a fake ring stands in for the queue.  Also the batch plan (step_plan.hpp) every step-kernel path runs by,
// against the launch counts the GPU tests pin.  Prints "aql packet test ok" on success (tests/test_aql_packets.py).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "aql_chain.hpp"
#include "step_plan.hpp"

using namespace sixdof;
using namespace sixdof::aql;

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                     \
        }                                                                     \
    } while (0)

namespace {

// A ring whose packet processor consumes every packet up to the last doorbell the moment the producer finds the ring
// full, recording what it consumed in order.
struct FakeQueue {
    std::vector<hsa_kernel_dispatch_packet_t> slots;
    uint64_t write = 0, read = 0, doorbell = UINT64_MAX, doorbells = 0, full_polls = 0;
    std::vector<hsa_kernel_dispatch_packet_t> consumed;

    explicit FakeQueue(uint64_t size, uint64_t start) : slots(size), write(start), read(start) {}
    void consume() {
        for (; doorbell != UINT64_MAX && read <= doorbell; read++) {
            hsa_kernel_dispatch_packet_t& p = slots[read & (slots.size() - 1)];
            CHECK((p.header & 0xff) == HSA_PACKET_TYPE_KERNEL_DISPATCH);   // a published packet
            consumed.push_back(p);
            p.header = HSA_PACKET_TYPE_INVALID;
        }
    }
    static uint64_t read_index(void* c) {
        auto* q = static_cast<FakeQueue*>(c);
        if (q->write - q->read == q->slots.size()) q->full_polls++, q->consume();
        return q->read;
    }
    static uint64_t reserve(void* c, uint64_t n) {
        auto* q = static_cast<FakeQueue*>(c);
        const uint64_t w = q->write;
        q->write += n;
        CHECK(q->write - q->read <= q->slots.size());   // never past the packets not yet read
        return w;
    }
    static void ring(void* c, uint64_t index) {
        auto* q = static_cast<FakeQueue*>(c);
        CHECK(index < q->write && (q->doorbell == UINT64_MAX || index > q->doorbell));
        q->doorbell = index;
        q->doorbells++;
    }
    Ring ring_view() { return Ring{slots.data(), slots.size(), this, read_index, reserve, ring}; }
};

void check_header(uint32_t hs, uint64_t i, uint64_t n) {
    const uint32_t header = hs & 0xffff, setup = hs >> 16;
    CHECK(((header >> HSA_PACKET_HEADER_TYPE) & 0xff) == HSA_PACKET_TYPE_KERNEL_DISPATCH);
    CHECK(((header >> HSA_PACKET_HEADER_BARRIER) & 1) == 1);
    const uint32_t acq = (header >> HSA_PACKET_HEADER_SCACQUIRE_FENCE_SCOPE) & 3;
    const uint32_t rel = (header >> HSA_PACKET_HEADER_SCRELEASE_FENCE_SCOPE) & 3;
    CHECK(acq == (i == 0 ? HSA_FENCE_SCOPE_SYSTEM : HSA_FENCE_SCOPE_AGENT));
    CHECK(rel == (i + 1 == n ? HSA_FENCE_SCOPE_SYSTEM : HSA_FENCE_SCOPE_AGENT));
    CHECK(setup == 1);   // one dimension
}

// Writes a chain of the given runs through a ring of `size` slots whose indices start at `start`; checks every packet.
void check_chain(uint64_t size, uint64_t start, const std::vector<Run>& runs) {
    FakeQueue q(size, start);
    uint64_t n = 0;
    for (const Run& r : runs) n += r.count;
    const hsa_signal_t first{0x1000}, last{0x2000};
    CHECK(write_chain(q.ring_view(), runs.data(), runs.size(), first, last, 1.0));
    q.consume();
    CHECK(q.consumed.size() == n);
    CHECK(q.read == start + n && q.write == start + n);
    if (n <= size) CHECK(q.doorbells == 1);   // one doorbell when the chain fits
    else CHECK(q.full_polls > 0);             // flow control took place
    uint64_t i = 0;
    for (const Run& r : runs) {
        for (uint64_t k = 0; k < r.count; k++, i++) {
            const hsa_kernel_dispatch_packet_t& p = q.consumed[i];
            check_header(uint32_t(p.header) | uint32_t(p.setup) << 16, i, n);
            CHECK(p.workgroup_size_x == 64 && p.workgroup_size_y == 1 && p.workgroup_size_z == 1);
            CHECK(p.grid_size_x == 64u * r.blocks && p.grid_size_y == 1 && p.grid_size_z == 1);   // work-items
            CHECK(p.private_segment_size == r.code.private_size && p.group_segment_size == r.code.group_size);
            CHECK(p.kernel_object == r.code.object);
            CHECK(p.kernarg_address == r.kernarg);
            CHECK(reinterpret_cast<uintptr_t>(p.kernarg_address) % r.code.kernarg_align == 0);
            const uint64_t want = i + 1 == n ? last.handle : i == 0 ? first.handle : 0;
            CHECK(p.completion_signal.handle == want);
        }
    }
}

struct Batch {
    uint64_t ticks, launches, graph_launches;
};

// A ladder of batches on one handle with K ticks per launch, as the GPU tests run it: `check[i]`, batch i opens with the
// accel-check launch.  The hipGraph and AQL paths count what the plan replays as graph_launches, an eager handle nothing.
void check_ladder(uint32_t K, const std::vector<Batch>& ladder, const std::vector<bool>& check) {
    for (size_t i = 0; i < ladder.size(); i++) {
        const Batch& x = ladder[i];
        const BatchPlan b = plan_batch(x.ticks, K, check[i], true);
        CHECK(b.launches() == x.launches && b.chains.launches() == x.graph_launches);
        CHECK(b.check_ticks + b.full * K + b.rem == x.ticks && b.rem < K && b.chains.launches() <= b.full);
        CHECK((b.check_ticks != 0) == check[i]);
        const BatchPlan eager = plan_batch(x.ticks, K, check[i], false);
        CHECK(eager.launches() == x.launches && eager.chains.launches() == 0);
    }
}

void check_chains(uint64_t full, bool open, uint64_t n_long, uint64_t n_short, uint32_t tail) {
    const ChainPlan c = plan_chains(full);
    CHECK(c.open == open && c.n_long == n_long && c.n_short == n_short && c.tail == tail);
}

void check_plans() {
    // tests/test_gpu_graph_replay.py K1_LADDER and K4_LADDER: only the first batch after the upload opens with the check launch
    const std::vector<Batch> k1 = {{40, 40, 39},    {3, 3, 0},       {4, 4, 4},       {20, 20, 20},    {35, 35, 32},
                                   {36, 36, 36},    {543, 543, 543}, {547, 547, 544}, {600, 600, 600}, {4099, 4099, 4096}};
    std::vector<bool> first(k1.size(), false);
    first[0] = true;
    check_ladder(1, k1, first);
    check_ladder(4, {{8, 2, 0}, {103, 26, 25}}, {true, false});
    // tests/test_gpu_aql_chain.py K8_TICKS: -(-n // 8) launches; the test uploads before entries 0 and 9
    const uint64_t k8[] = {20, 17, 18, 19, 21, 22, 23, 5, 3, 100, 7, 23, 61, 8, 30, 1, 4099};
    for (size_t i = 0; i < sizeof(k8) / sizeof(k8[0]); i++) {
        const BatchPlan b = plan_batch(k8[i], 8, i == 0 || i == 9, true);
        CHECK(b.launches() == (k8[i] + 7) / 8 && b.check_ticks + b.full * 8 + b.rem == k8[i]);
    }
    CHECK(plan_batch(5, 8, true, true).check_ticks == 5 && plan_batch(0, 8, true, true).launches() == 0);
    // the chains behind those counts: an opening 32-launch chain from 544 launches on, tails of at least kGraphMinLen
    check_chains(39, false, 0, 1, 7);
    check_chains(3, false, 0, 0, 0);
    check_chains(4, false, 0, 0, 4);
    check_chains(543, false, 0, 16, 31);
    check_chains(544, true, 4, 0, 0);
    check_chains(600, true, 4, 1, 24);
    check_chains(4099, true, 31, 3, 0);
}

}  // namespace

int main() {
    check_plans();
    CHECK(sizeof(hsa_kernel_dispatch_packet_t) == 64);
    for (uint64_t n : {1u, 2u, 3u, 20u, 4096u})
        for (uint64_t i = 0; i < n; i++) check_header(header_setup(i, n), i, n);

    alignas(256) static char args[3][2560];
    const KernelCode main_k{0xabc000, 2440, 16, 12544, 0}, check_k{0xdef000, 2440, 16, 12544, 64};
    const Run check{check_k, args[0], 1024, 1}, chain{main_k, args[1], 1024, 20}, rem{main_k, args[2], 1024, 1};
    check_chain(1024, 0, {chain});                     // the benchmark's batch
    check_chain(1024, 0, {check, chain, rem});         // accel-check launch, chain, remainder
    check_chain(16, 10, {check, chain, rem});          // wraps the ring twice, with flow control
    check_chain(1024, 1000, {Run{main_k, args[1], 1024, 4096}});   // 4,096 launches through a 1,024-slot ring
    check_chain(64, 60, {Run{main_k, args[1], 7, 1}}); // one packet: first and last at once
    check_chain(64, 0, {Run{main_k, args[1], 7, 0}, chain, Run{check_k, args[0], 7, 0}});   // empty runs are skipped

    // a ring that never drains: write_chain gives up after its timeout instead of overwriting unread packets
    FakeQueue stuck(8, 0);
    Ring r = stuck.ring_view();
    r.read_index = [](void*) -> uint64_t { return 0; };
    const Run many{main_k, args[1], 1, 9};
    CHECK(!write_chain(r, &many, 1, hsa_signal_t{1}, hsa_signal_t{2}, 0.01));
    CHECK(stuck.write == 8 && stuck.doorbell == 7);   // the 8 packets that fit were published before the wait
    std::printf("aql packet test ok\n");
    return 0;
}
