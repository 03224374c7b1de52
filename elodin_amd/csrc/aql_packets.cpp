// aql_packets.cpp — the packet builder of aql_chain.hpp: pure host code (no HSA calls), built into the library and into
// the host unit test (make aql_test).
#include <chrono>
#include <cstring>

#include "aql_chain.hpp"

namespace sixdof::aql {

uint32_t header_setup(uint64_t i, uint64_t n) {
    const uint32_t acquire = i == 0 ? HSA_FENCE_SCOPE_SYSTEM : HSA_FENCE_SCOPE_AGENT;
    const uint32_t release = i + 1 == n ? HSA_FENCE_SCOPE_SYSTEM : HSA_FENCE_SCOPE_AGENT;
    const uint32_t header = (HSA_PACKET_TYPE_KERNEL_DISPATCH << HSA_PACKET_HEADER_TYPE) | (1u << HSA_PACKET_HEADER_BARRIER) |
                            (acquire << HSA_PACKET_HEADER_SCACQUIRE_FENCE_SCOPE) |
                            (release << HSA_PACKET_HEADER_SCRELEASE_FENCE_SCOPE);
    const uint32_t setup = 1u << HSA_KERNEL_DISPATCH_PACKET_SETUP_DIMENSIONS;
    return header | setup << 16;
}

void fill_body(hsa_kernel_dispatch_packet_t* p, const KernelCode& k, uint32_t blocks, const void* kernarg, hsa_signal_t signal) {
    // everything after the first 32 bits: the header is published last, by write_chain
    std::memset(reinterpret_cast<char*>(p) + 4, 0, sizeof(*p) - 4);
    p->workgroup_size_x = kWorkgroup;
    p->workgroup_size_y = 1;
    p->workgroup_size_z = 1;
    p->grid_size_x = static_cast<uint32_t>(kWorkgroup) * blocks;
    p->grid_size_y = 1;
    p->grid_size_z = 1;
    p->private_segment_size = k.private_size;
    p->group_segment_size = k.group_size;
    p->kernel_object = k.object;
    p->kernarg_address = const_cast<void*>(kernarg);
    p->completion_signal = signal;
}

bool write_chain(const Ring& r, const Run* runs, size_t n_runs, hsa_signal_t first, hsa_signal_t last, double timeout_s) {
    uint64_t n = 0;
    for (size_t i = 0; i < n_runs; i++) n += runs[i].count;
    if (n == 0) return true;
    const hsa_signal_t none{0};
    size_t run = 0;
    uint64_t in_run = 0;   // packets of runs[run] already written
    uint64_t done = 0;
    while (done < n) {
        // flow control: reserve only slots the packet processor has already read.  The wait starts when the ring is full
        // and ends as soon as one packet is read, so it gives up only on a queue that stopped moving, never on a long chain
        uint64_t room = r.size - (r.reserve(r.ctx, 0) - r.read_index(r.ctx));
        const auto deadline = std::chrono::steady_clock::now() + std::chrono::duration<double>(timeout_s);
        while (room == 0) {
            if (std::chrono::steady_clock::now() > deadline) return false;
            room = r.size - (r.reserve(r.ctx, 0) - r.read_index(r.ctx));
        }
        const uint64_t m = n - done < room ? n - done : room;
        const uint64_t w = r.reserve(r.ctx, m);
        for (uint64_t j = 0; j < m; j++) {
            while (in_run == runs[run].count) run++, in_run = 0;
            const Run& R = runs[run];
            const uint64_t i = done + j;
            const hsa_signal_t sig = i + 1 == n ? last : i == 0 ? first : none;
            fill_body(&r.base[(w + j) & (r.size - 1)], R.code, R.blocks, R.kernarg, sig);
            in_run++;
        }
        for (uint64_t j = 0; j < m; j++)
            __atomic_store_n(reinterpret_cast<uint32_t*>(&r.base[(w + j) & (r.size - 1)]), header_setup(done + j, n), __ATOMIC_RELEASE);
        done += m;
        r.doorbell(r.ctx, w + m - 1);
    }
    return true;
}

}  // namespace sixdof::aql
