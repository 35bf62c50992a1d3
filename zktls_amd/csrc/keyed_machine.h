// keyed_machine.h -- what a machine with an order array hands the five keyed-machine entries (zkhip_machine_setup, zkhip_machine_key_host,
// zkhip_machine_proof_size_keyed, zkhip_prove_machine_keyed, zkhip_verify_machine_keyed): ONE struct with the arrays those entries take, by
// POSITION, and plain functions over it.  The shard verifier (rec), the machine verifier (mrec) and the five fold-16 machines (fri16) number their
// chips as they like and keep their own shape, cache key and cache policy; what is by position is here.
//   position: where a chip stands in the machine -- tallest first, equal heights in chip-number order (a stable sort: the one in build below)
// Uploading preprocessed tables stays with the caller (one staging block for the verifiers, a scratch slot per table for fri16); key_setup takes
// device pointers.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "babybear.cuh"
#include "context.h"

namespace zk {
namespace keyed {

constexpr int MAX_CHIPS = 16;
struct KeyedMachine {
    int n = 0;
    int order[MAX_CHIPS];                                               // position -> chip number
    int height[MAX_CHIPS]; uint32_t w_main[MAX_CHIPS], w_pre[MAX_CHIPS];     // by chip number: log2 of the rows, main width, preprocessed width
    int32_t log_ns[MAX_CHIPS]; uint32_t widths[MAX_CHIPS], pre_widths[MAX_CHIPS];      // the same by position
    std::vector<uint32_t> prog[MAX_CHIPS], tab[MAX_CHIPS];              // by position: the chip's program and interaction table
    const uint32_t* progs[MAX_CHIPS]; size_t prog_words[MAX_CHIPS]; const uint32_t* tabs[MAX_CHIPS]; size_t tab_words[MAX_CHIPS];
    KeyedMachine() = default;
    KeyedMachine(const KeyedMachine&) = delete;                         // (progs / tabs point into prog / tab)
    KeyedMachine& operator=(const KeyedMachine&) = delete;
    int pos_of(int chip) const { for (int i = 0; i < n; i++) if (order[i] == chip) return i; return -1; }
};

// fill(chip, program, table) writes chip's program and interaction table; it is called in machine order
template <class Fill>
void build(KeyedMachine& m, int n, const int* height, const uint32_t* w_main, const uint32_t* w_pre, Fill fill) {
    m.n = n;
    for (int c = 0; c < n; c++) { m.order[c] = c; m.height[c] = height[c]; m.w_main[c] = w_main[c]; m.w_pre[c] = w_pre[c]; }
    std::stable_sort(m.order, m.order + n, [&](int a, int b) { return height[a] > height[b]; });
    for (int i = 0; i < n; i++) {
        const int c = m.order[i];
        fill(c, m.prog[i], m.tab[i]);
        m.log_ns[i] = height[c]; m.widths[i] = w_main[c]; m.pre_widths[i] = w_pre[c];
        m.progs[i] = m.prog[i].data(); m.prog_words[i] = m.prog[i].size(); m.tabs[i] = m.tab[i].data(); m.tab_words[i] = m.tab[i].size();
    }
}

inline size_t proof_size(const KeyedMachine& m, const zkhip_params* prm, size_t n_public) {
    return zkhip_machine_proof_size_keyed(m.log_ns, m.widths, m.pre_widths, m.progs, m.prog_words, m.tabs, m.tab_words, m.n, prm, n_public);
}
inline int verify(const KeyedMachine& m, const uint8_t* proof, size_t len, const uint32_t vk[8], const uint32_t* public_values, size_t n_public, const zkhip_params* prm, int* reason) {
    return zkhip_verify_machine_keyed(proof, len, m.log_ns, m.widths, m.pre_widths, vk, m.progs, m.prog_words, m.tabs, m.tab_words, m.n, public_values, n_public, prm, reason);
}
// d_traces: the main traces on the device (dense), by chip number
inline int prove(zkhip_ctx* ctx, const zkhip_machine_key* key, const KeyedMachine& m, const uint32_t* const* d_traces, const uint32_t* public_values, size_t n_public,
                 const zkhip_params* prm, uint8_t* proof, size_t cap, size_t* len) {
    zkhip_chip chips[MAX_CHIPS]{};
    for (int i = 0; i < m.n; i++) { chips[i].d_trace = d_traces[m.order[i]]; chips[i].ld = m.widths[i]; chips[i].log_n = m.log_ns[i]; chips[i].width = m.widths[i]; chips[i].partner = -1; }
    return zkhip_prove_machine_keyed(ctx, key, chips, m.progs, m.prog_words, m.tabs, m.tab_words, m.n, public_values, n_public, prm, proof, cap, len);
}
// pre: the preprocessed traces by chip number (host, Montgomery); an empty one: the chip has none (a null pointer and width 0)
inline int key_host(const KeyedMachine& m, const std::vector<uint32_t>* pre, const zkhip_params* prm, uint32_t vk[8]) {
    const uint32_t* traces[MAX_CHIPS]; uint32_t pws[MAX_CHIPS];
    for (int i = 0; i < m.n; i++) {
        const std::vector<uint32_t>& t = pre[m.order[i]];
        traces[i] = t.empty() ? nullptr : t.data(); pws[i] = t.empty() ? 0u : m.pre_widths[i];
    }
    return zkhip_machine_key_host(traces, m.log_ns, pws, m.n, prm, vk);
}
// d_pre: the same traces on the device, by chip number (null: none); the key keeps its own copies
inline int key_setup(zkhip_ctx* ctx, const KeyedMachine& m, const uint32_t* const* d_pre, const zkhip_params* prm, zkhip_machine_key** key, uint32_t vk[8]) {
    zkhip_chip chips[MAX_CHIPS]{};
    for (int i = 0; i < m.n; i++) { chips[i].d_trace = d_pre[m.order[i]]; chips[i].log_n = m.log_ns[i]; chips[i].width = m.pre_widths[i]; chips[i].ld = m.pre_widths[i]; chips[i].partner = -1; }
    return zkhip_machine_setup(ctx, chips, m.n, prm, key, vk);
}
// the machine as data: position `which`; what 0 = the chip's program, 1 = its interaction table, 2 = its preprocessed trace in canonical words, row-major, which
// pre_of(chip, log_rows, out) builds in Montgomery form (nothing: the chip has none).  Returns the word count (0: no such position or kind); out may be null
template <class PreOf>
size_t describe(const KeyedMachine& m, int which, int what, PreOf pre_of, uint32_t* out, size_t cap_words, int* log_rows, uint32_t* main_width, uint32_t* pre_width) {
    if (which < 0 || which >= m.n || what < 0 || what > 2) return 0;
    if (log_rows) *log_rows = m.log_ns[which];
    if (main_width) *main_width = m.widths[which];
    if (pre_width) *pre_width = m.pre_widths[which];
    std::vector<uint32_t> pre;
    if (what == 2) {
        pre_of(m.order[which], (int)m.log_ns[which], pre);
        for (uint32_t& v : pre) v = from_monty(v);
    }
    const std::vector<uint32_t>& src = what == 0 ? m.prog[which] : what == 1 ? m.tab[which] : pre;
    if (out && cap_words >= src.size()) std::memcpy(out, src.data(), src.size() * 4);
    return src.size();
}

}  // namespace keyed
}  // namespace zk
