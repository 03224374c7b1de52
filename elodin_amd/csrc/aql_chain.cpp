// aql_chain.cpp — the HSA side of aql_chain.hpp: one queue per device and process, the step kernels' code looked up in
// the library's own gfx950 code object, chain submission and the completion wait.
#include <dlfcn.h>
#include <elf.h>
#include <hip/hip_runtime.h>
#include <hsa/hsa_ext_amd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "aql_chain.hpp"

namespace sixdof::aql {

namespace {

constexpr uint32_t kRingSlots = 1024;   // power of two; a longer chain is flow-controlled on the read index
constexpr char kBundleMagic[] = "__CLANG_OFFLOAD_BUNDLE__";
constexpr char kTarget[] = "hipv4-amdgcn-amd-amdhsa--gfx950";

}  // namespace

struct Device {
    int hip_device = 0;
    int refs = 0;
    hsa_agent_t agent{};
    hsa_queue_t* queue = nullptr;
    hsa_signal_t first{}, last{};
    std::atomic<int> queue_status{HSA_STATUS_SUCCESS};   // set by the queue's error callback
    std::string fault;                                   // why chains are refused (queue error or timeout)
    std::vector<char> library;                           // this library's file: its offload bundles
    std::map<size_t, hsa_executable_t> executables;      // code object (offset in `library`) -> loaded executable
    std::map<const void*, KernelCode> kernels;
    std::mutex m;   // one chain at a time on the queue
};

namespace {

std::mutex g_devices_mutex;
std::map<int, Device*> g_devices;

std::string hsa_error(const char* what, hsa_status_t s) {
    const char* msg = nullptr;
    if (hsa_status_string(s, &msg) != HSA_STATUS_SUCCESS || !msg) msg = "unknown HSA status";
    return std::string(what) + ": " + msg;
}

void on_queue_error(hsa_status_t status, hsa_queue_t*, void* data) {
    // record only: the next chain (and every later one) reports it; nothing is resubmitted
    static_cast<Device*>(data)->queue_status.store(status);
}

struct AgentQuery {
    uint32_t domain, bdf;
    std::vector<hsa_agent_t> found;
};

hsa_status_t match_agent(hsa_agent_t a, void* data) {
    auto* q = static_cast<AgentQuery*>(data);
    hsa_device_type_t type;
    if (hsa_agent_get_info(a, HSA_AGENT_INFO_DEVICE, &type) != HSA_STATUS_SUCCESS || type != HSA_DEVICE_TYPE_GPU)
        return HSA_STATUS_SUCCESS;
    uint32_t bdf = 0, domain = 0;
    if (hsa_agent_get_info(a, static_cast<hsa_agent_info_t>(HSA_AMD_AGENT_INFO_BDFID), &bdf) != HSA_STATUS_SUCCESS ||
        hsa_agent_get_info(a, static_cast<hsa_agent_info_t>(HSA_AMD_AGENT_INFO_DOMAIN), &domain) != HSA_STATUS_SUCCESS)
        return HSA_STATUS_SUCCESS;
    if (bdf == q->bdf && domain == q->domain) q->found.push_back(a);
    return HSA_STATUS_SUCCESS;
}

void destroy(Device* d) {
    if (d->queue) hsa_queue_destroy(d->queue);
    if (d->first.handle) hsa_signal_destroy(d->first);
    if (d->last.handle) hsa_signal_destroy(d->last);
    for (auto& kv : d->executables) hsa_executable_destroy(kv.second);
    delete d;
    hsa_shut_down();
}

bool setup(Device* d, std::string* why) {
    // under rocprofv3 every queue is an intercept queue, and the tool's packet rewrite faulted (SIGSEGV on the host) on
    // the first doorbell of a chain: keep the hipGraph path, which the profiler handles, while it is loaded
    for (const char* tool : {"librocprofiler-sdk.so.1", "librocprofiler-sdk.so"}) {
        if (void* lib = dlopen(tool, RTLD_NOW | RTLD_NOLOAD)) {
            dlclose(lib);
            return *why = std::string(tool) + " is loaded (profiler queue interception)", false;
        }
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, d->hip_device) != hipSuccess) return *why = "hipGetDeviceProperties failed", false;
    // the HSA agent of the HIP device: same PCI domain and bus/device/function id (function 0 of the device)
    AgentQuery q{static_cast<uint32_t>(prop.pciDomainID), static_cast<uint32_t>(prop.pciBusID << 8 | prop.pciDeviceID << 3), {}};
    hsa_status_t s = hsa_iterate_agents(match_agent, &q);
    if (s != HSA_STATUS_SUCCESS) return *why = hsa_error("hsa_iterate_agents", s), false;
    if (q.found.size() != 1)
        return *why = "no single HSA agent has the HIP device's PCI id (" + std::to_string(q.found.size()) + " match)", false;
    d->agent = q.found[0];
    if ((s = hsa_queue_create(d->agent, kRingSlots, HSA_QUEUE_TYPE_SINGLE, on_queue_error, d, UINT32_MAX, UINT32_MAX,
                              &d->queue)) != HSA_STATUS_SUCCESS)
        return d->queue = nullptr, *why = hsa_error("hsa_queue_create", s), false;
    if ((s = hsa_amd_profiling_set_profiler_enabled(d->queue, 1)) != HSA_STATUS_SUCCESS)
        return *why = hsa_error("hsa_amd_profiling_set_profiler_enabled", s), false;
    if ((s = hsa_signal_create(1, 0, nullptr, &d->first)) != HSA_STATUS_SUCCESS ||
        (s = hsa_signal_create(1, 0, nullptr, &d->last)) != HSA_STATUS_SUCCESS)
        return *why = hsa_error("hsa_signal_create", s), false;
    // this library's file: the code objects HIP loads come from its offload bundles
    Dl_info info{};
    if (!dladdr(reinterpret_cast<const void*>(&acquire), &info) || !info.dli_fname)
        return *why = "dladdr: cannot find the library file", false;
    std::ifstream f(info.dli_fname, std::ios::binary);
    d->library.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    if (d->library.empty()) return *why = std::string("cannot read ") + info.dli_fname, false;
    return true;
}

// The gfx950 code objects of every offload bundle in the library's .hip_fatbin section: (offset, size) in the file.
std::vector<std::pair<size_t, size_t>> gfx950_code_objects(const std::vector<char>& lib) {
    std::vector<std::pair<size_t, size_t>> out;
    if (lib.size() < sizeof(Elf64_Ehdr)) return out;
    Elf64_Ehdr eh;
    std::memcpy(&eh, lib.data(), sizeof(eh));
    if (std::memcmp(eh.e_ident, ELFMAG, SELFMAG) != 0 || eh.e_shoff + size_t(eh.e_shnum) * sizeof(Elf64_Shdr) > lib.size() ||
        eh.e_shstrndx >= eh.e_shnum)
        return out;
    auto shdr = [&](size_t i) {
        Elf64_Shdr s;
        std::memcpy(&s, lib.data() + eh.e_shoff + i * sizeof(Elf64_Shdr), sizeof(s));
        return s;
    };
    const Elf64_Shdr names = shdr(eh.e_shstrndx);
    for (size_t i = 0; i < eh.e_shnum; i++) {
        const Elf64_Shdr s = shdr(i);
        if (names.sh_offset + s.sh_name + 12 > lib.size() || std::strcmp(lib.data() + names.sh_offset + s.sh_name, ".hip_fatbin") != 0)
            continue;
        if (s.sh_offset + s.sh_size > lib.size()) return out;
        // one bundle per translation unit: magic, entry count, then (offset, size, triple length, triple) per entry
        const char* sec = lib.data() + s.sh_offset;
        for (size_t b = 0; b + 32 <= s.sh_size; b += 8) {
            if (std::memcmp(sec + b, kBundleMagic, 24) != 0) continue;
            uint64_t n = 0;
            std::memcpy(&n, sec + b + 24, 8);
            size_t e = b + 32;
            for (uint64_t k = 0; k < n && e + 24 <= s.sh_size; k++) {
                uint64_t off, size, tl;
                std::memcpy(&off, sec + e, 8);
                std::memcpy(&size, sec + e + 8, 8);
                std::memcpy(&tl, sec + e + 16, 8);
                e += 24;
                if (e + tl > s.sh_size) break;
                if (std::string(sec + e, tl) == kTarget && b + off + size <= s.sh_size) out.emplace_back(s.sh_offset + b + off, size);
                e += tl;
            }
        }
    }
    return out;
}

bool contains(const char* p, size_t n, const std::string& needle) {
    return std::search(p, p + n, needle.begin(), needle.end()) != p + n;
}

}  // namespace

Device* acquire(int hip_device, std::string* why) {
    std::lock_guard<std::mutex> lock(g_devices_mutex);
    auto it = g_devices.find(hip_device);
    if (it != g_devices.end()) {
        it->second->refs++;
        return it->second;
    }
    hsa_status_t s = hsa_init();
    if (s != HSA_STATUS_SUCCESS) return *why = hsa_error("hsa_init", s), nullptr;
    auto* d = new Device();
    d->hip_device = hip_device;
    if (!setup(d, why)) {
        destroy(d);
        return nullptr;
    }
    d->refs = 1;
    g_devices[hip_device] = d;
    return d;
}

void release(Device* d) {
    if (!d) return;
    std::lock_guard<std::mutex> lock(g_devices_mutex);
    if (--d->refs > 0) return;
    g_devices.erase(d->hip_device);
    destroy(d);
}

bool kernel_code(Device* d, const void* stub, uint32_t explicit_kernarg_bytes, KernelCode* out, std::string* why) {
    std::lock_guard<std::mutex> lock(d->m);
    if (auto it = d->kernels.find(stub); it != d->kernels.end()) return *out = it->second, true;
    // the kernel's mangled name: HIP names a kernel's host handle after the kernel
    Dl_info info{};
    if (!dladdr(stub, &info) || !info.dli_sname || info.dli_saddr != stub) return *why = "dladdr: the kernel's host handle has no symbol", false;
    const std::string name = std::string(info.dli_sname) + ".kd";
    for (const auto& [off, size] : gfx950_code_objects(d->library)) {
        if (!contains(d->library.data() + off, size, std::string(1, '\0') + name + '\0')) continue;
        auto ex = d->executables.find(off);
        if (ex == d->executables.end()) {
            hsa_code_object_reader_t reader;
            hsa_executable_t exe;
            hsa_status_t s = hsa_code_object_reader_create_from_memory(d->library.data() + off, size, &reader);
            if (s != HSA_STATUS_SUCCESS) return *why = hsa_error("hsa_code_object_reader_create_from_memory", s), false;
            s = hsa_executable_create_alt(HSA_PROFILE_FULL, HSA_DEFAULT_FLOAT_ROUNDING_MODE_DEFAULT, nullptr, &exe);
            if (s == HSA_STATUS_SUCCESS) {
                s = hsa_executable_load_agent_code_object(exe, d->agent, reader, nullptr, nullptr);
                if (s == HSA_STATUS_SUCCESS) s = hsa_executable_freeze(exe, nullptr);
                if (s != HSA_STATUS_SUCCESS) hsa_executable_destroy(exe);
            }
            hsa_code_object_reader_destroy(reader);
            if (s != HSA_STATUS_SUCCESS) return *why = hsa_error("loading the library's gfx950 code object", s), false;
            ex = d->executables.emplace(off, exe).first;
        }
        hsa_executable_symbol_t sym;
        if (hsa_executable_get_symbol_by_name(ex->second, name.c_str(), &d->agent, &sym) != HSA_STATUS_SUCCESS) continue;
        KernelCode k;
        bool dynamic_stack = true;
        hsa_status_t s = hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_OBJECT, &k.object);
        if (s == HSA_STATUS_SUCCESS) s = hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_KERNARG_SEGMENT_SIZE, &k.kernarg_size);
        if (s == HSA_STATUS_SUCCESS) s = hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_KERNARG_SEGMENT_ALIGNMENT, &k.kernarg_align);
        if (s == HSA_STATUS_SUCCESS) s = hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_GROUP_SEGMENT_SIZE, &k.group_size);
        if (s == HSA_STATUS_SUCCESS) s = hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_PRIVATE_SEGMENT_SIZE, &k.private_size);
        if (s == HSA_STATUS_SUCCESS) s = hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_DYNAMIC_CALLSTACK, &dynamic_stack);
        if (s != HSA_STATUS_SUCCESS) return *why = hsa_error("hsa_executable_symbol_get_info", s), false;
        // hidden arguments sit after the explicit ones: a larger segment means the metadata lists some, which a HIP
        // launch fills and this path does not
        if (k.kernarg_size != explicit_kernarg_bytes)
            return *why = name + ": kernarg segment of " + std::to_string(k.kernarg_size) + " bytes, " +
                          std::to_string(explicit_kernarg_bytes) + " explicit (hidden arguments)", false;
        if (dynamic_stack) return *why = name + ": dynamic call stack", false;
        d->kernels[stub] = k;
        return *out = k, true;
    }
    return *why = name + ": not found in the library's gfx950 code objects", false;
}

namespace {

uint64_t ring_read_index(void* q) { return hsa_queue_load_read_index_scacquire(static_cast<hsa_queue_t*>(q)); }
uint64_t ring_reserve(void* q, uint64_t n) { return hsa_queue_add_write_index_scacq_screl(static_cast<hsa_queue_t*>(q), n); }
void ring_doorbell(void* q, uint64_t index) {
    hsa_signal_store_screlease(static_cast<hsa_queue_t*>(q)->doorbell_signal, static_cast<hsa_signal_value_t>(index));
}

}  // namespace

bool run_chain(Device* d, const Run* runs, size_t n_runs, double stall_s, double* device_ms, std::string* why) {
    std::lock_guard<std::mutex> lock(d->m);
    if (d->fault.empty() && d->queue_status.load() != HSA_STATUS_SUCCESS)
        d->fault = hsa_error("AQL queue error", static_cast<hsa_status_t>(d->queue_status.load()));
    if (!d->fault.empty()) return *why = d->fault, false;
    uint64_t n = 0;
    for (size_t i = 0; i < n_runs; i++) n += runs[i].count;
    *device_ms = 0.0;
    if (n == 0) return true;
    hsa_signal_store_relaxed(d->first, 1);
    hsa_signal_store_relaxed(d->last, 1);
    const hsa_signal_t first = n == 1 ? d->last : d->first;
    const Ring ring{static_cast<hsa_kernel_dispatch_packet_t*>(d->queue->base_address), d->queue->size, d->queue,
                    ring_read_index, ring_reserve, ring_doorbell};
    if (!write_chain(ring, runs, n_runs, first, d->last, stall_s))
        return *why = d->fault = "AQL chain: the queue read no packet for " + std::to_string(stall_s) + " s", false;
    // active spin: a batch is tens of microseconds; a blocking wait's wake-up would cost as much again.  The limit is on
    // progress, not on the chain's length: every packet the packet processor reads restarts it (with the barrier bit it
    // reads the next one once the previous launch is done), so only a launch that runs stall_s by itself ends the wait
    uint64_t seen = hsa_queue_load_read_index_relaxed(d->queue);
    auto deadline = std::chrono::steady_clock::now() + std::chrono::duration<double>(stall_s);
    while (hsa_signal_load_scacquire(d->last) != 0) {
        if (d->queue_status.load() != HSA_STATUS_SUCCESS)
            return *why = d->fault = hsa_error("AQL queue error", static_cast<hsa_status_t>(d->queue_status.load())), false;
        const auto now = std::chrono::steady_clock::now();
        if (const uint64_t read = hsa_queue_load_read_index_relaxed(d->queue); read != seen) {
            seen = read;
            deadline = now + std::chrono::duration<double>(stall_s);
        } else if (now > deadline) {
            return *why = d->fault = "AQL chain: no progress for " + std::to_string(stall_s) + " s", false;
        }
    }
    hsa_amd_profiling_dispatch_time_t a{}, b{};
    if (hsa_amd_profiling_get_dispatch_time(d->agent, first, &a) == HSA_STATUS_SUCCESS &&
        hsa_amd_profiling_get_dispatch_time(d->agent, d->last, &b) == HSA_STATUS_SUCCESS && b.end > a.start)
        *device_ms = static_cast<double>(b.end - a.start) * 1e-6;
    return true;
}

}  // namespace sixdof::aql
