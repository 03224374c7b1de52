// capi_fake_program.cpp — a host-only object with the entry points of a generated program (elodin_amd/codegen.py), for
// capi_lifecycle_test.cpp: no aux column, one component column, one fold stage that reads its edges from a device table.
// Its launch computes nothing, but it reads every table it was handed — with the fake runtime device memory is host
// memory, so AddressSanitizer reports a table that was freed or is too short.
#include <cstdint>

#include "kernels.hpp"

namespace {
// what a generated object carries of its own (codegen.py _FOLD_TABLE); the host layer checks the size it reports
struct FoldTable {
    const uint32_t* src_rows;
    const uint32_t* row_start;
    const uint32_t* dst;
    uint32_t n_src;
    uint32_t n_lane;
};
const FoldTable* g_table = nullptr;
volatile uint64_t g_sink;
}  // namespace

extern "C" {
unsigned sixdof_custom_abi() { return sizeof(sixdof::StepParams); }
unsigned sixdof_custom_layout() { return 0u | 1u << 8; }   // n_aux | n_model_cols << 8
unsigned sixdof_custom_fold_count() { return 1; }
int sixdof_custom_fold_info(unsigned fold, unsigned* out) {
    if (fold != 0) return 1;
    out[0] = 1u, out[1] = 1u, out[2] = 0u, out[3] = sizeof(FoldTable);   // needs a table; no replicas
    return 0;
}
int sixdof_custom_set_fold_table(unsigned fold, const FoldTable* t) { return fold == 0 ? (g_table = t, 0) : 1; }
int sixdof_custom_launch(const sixdof::StepParams* p, int, int, void*) {
    uint64_t sum = 0;
    if (const FoldTable* t = g_table) {
        for (uint32_t i = 0; i < t->n_src; i++) sum += t->src_rows[i];
        for (uint32_t i = 0; i <= t->n_src; i++) sum += t->row_start[i];
        for (uint32_t e = 0; e < t->row_start[t->n_src]; e++) sum += t->dst[e];
    }
    const size_t n = p->n;
    if (n) sum += static_cast<const unsigned char*>(p->pos)[n * 7 * 8 - 1] + static_cast<const unsigned char*>(p->model_cols[0])[n * 8 - 1];
    if (n && p->hist_ring) sum += static_cast<const unsigned char*>(p->hist_pos)[size_t(p->hist_ring) * n * 7 * 8 - 1] + static_cast<const unsigned char*>(p->model_hist[0])[size_t(p->hist_ring) * n * 8 - 1];
    g_sink = sum;
    return 0;   // hipSuccess
}
}  // extern "C"
