// aql_chain.hpp — a batch of step-kernel launches written straight into an HSA queue the library owns.
//
// Every launch of a replayed chain has the same kernel object, grid and argument block (sixdof_capi.cpp Replay::key),
// so a batch needs none of the graph-replay machinery: its launches are written as kernel-dispatch packets that share
// pre-built argument blocks in device memory, the doorbell is rung once, and the host spins on the last packet's
// completion signal.  The packet layout (header bits, fence scopes by position, ring wrap-around and flow control) is
// pure host code, unit-tested without a GPU (aql_packet_test.cpp); the queue, the code-object lookup and the signals
// are in aql_chain.cpp.
#pragma once

#include <hsa/hsa.h>

#include <cstdint>
#include <string>

namespace sixdof::aql {

constexpr uint16_t kWorkgroup = 64;   // the step kernel's workgroup: one wave (step_kernel.hpp kWave)

// A kernel as the packet processor dispatches it: the code object's kernel descriptor and its segment sizes.
struct KernelCode {
    uint64_t object = 0;
    uint32_t kernarg_size = 0, kernarg_align = 0, group_size = 0, private_size = 0;
};

// `count` consecutive launches of one kernel with one argument block (device memory, `code.kernarg_size` bytes).
struct Run {
    KernelCode code;
    const void* kernarg = nullptr;
    uint32_t blocks = 0;    // workgroups of kWorkgroup threads
    uint64_t count = 0;
};

// header | setup << 16 of packet `i` of an `n`-packet chain: kernel dispatch, barrier bit, one dimension; system-scope
// acquire on the first packet (host uploads become visible), system-scope release on the last (the host and copy engines
// read the results), agent scope between launches of the chain.
uint32_t header_setup(uint64_t i, uint64_t n);

// Everything of a dispatch packet but its first 32 bits (header and setup): workgroup kWorkgroup x 1 x 1, grid in
// work-items (kWorkgroup * blocks), segment sizes from the kernel's symbol.
void fill_body(hsa_kernel_dispatch_packet_t* p, const KernelCode& k, uint32_t blocks, const void* kernarg, hsa_signal_t signal);

// A ring of `size` (power of two) packet slots and the three queue operations write_chain needs: the packet processor's
// read index, reserving slots (add to the write index, return the old one) and ringing the doorbell with the index of the
// last packet written.
struct Ring {
    hsa_kernel_dispatch_packet_t* base = nullptr;
    uint64_t size = 0;
    void* ctx = nullptr;
    uint64_t (*read_index)(void* ctx) = nullptr;
    uint64_t (*reserve)(void* ctx, uint64_t n) = nullptr;
    void (*doorbell)(void* ctx, uint64_t index) = nullptr;
};

// Writes the runs as one chain of packets: bodies first, then the headers in order with release stores.  `first` is
// the first packet's completion signal and `last` the last one's (the same signal for a one-packet chain).  The doorbell
// is rung once at the end, and also whenever the ring is full: a chain longer than the ring waits for the read index
// (flow control); it gives up when the read index has not moved for `timeout_s`, and returns false.
bool write_chain(const Ring& r, const Run* runs, size_t n_runs, hsa_signal_t first, hsa_signal_t last, double timeout_s);

// ---- the queue (aql_chain.cpp) --------------------------------------------------------------------------------

struct Device;   // one HSA queue per HIP device and process, shared by every handle on that device

// A reference to the process's queue on `hip_device`, created on first use (nullptr and *why on failure).
Device* acquire(int hip_device, std::string* why);
// Drops a reference; the last one destroys the queue, its signals and the loaded code objects.
void release(Device* d);

// The kernel a host stub (the address of a __global__ function) names, looked up in the library's own gfx950 code object.
// Fails (false, *why) when the kernel's argument block would need hidden arguments or a dynamic call stack: this path
// fills the explicit argument block only.
bool kernel_code(Device* d, const void* stub, uint32_t explicit_kernarg_bytes, KernelCode* out, std::string* why);

// Submits the runs as one chain and spins until the last packet completes.  It gives up only when the queue makes no
// progress (reads no packet) for `stall_s`, however long the chain.  *device_ms: first dispatch's start to last
// dispatch's end, from the packets' profiling timestamps.  Returns false with *why on a queue error or a stall; the queue
// then refuses every later chain.
bool run_chain(Device* d, const Run* runs, size_t n_runs, double stall_s, double* device_ms, std::string* why);

}  // namespace sixdof::aql
