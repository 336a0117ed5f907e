// Host emulation of phasm_amd/csrc/components.hip.h for tests/test_components_host_emulation.py: the kernels compiled as
// plain C++ with ONE lane per wave (threads run one after another), so a machine without a GPU checks their indexing and
// logic -- the sort of the rank words, the ranks of the edge ends, the hook and jump rounds, the numbering of the roots,
// the labels and the table -- against the goldens, under the host sanitizers.  The launches follow run_components
// (c_api.hip): the same memsets, and the round cap, the batches and the stop at the first round that lowers no word are
// round_phase of components.hip.h, which run_components itself launches by.  The workspaces start as a call before
// could have left them.  Every loop here and in the kernels is bounded by a count.
//   stdin:  n_total n_edges n_order, one "u v" line per edge, the nodes in node order (node ids < n_total; ids at or
//           above the reads are merged nodes: the kernels do not tell them apart)
//   stdout: "invalid N" alone, or: the counters order, components, singletons, max nodes, max edges, rounds, batches, cap;
//           the component of every rank; the component of every edge; per component "first_node n_nodes n_edges;"
#include "host_emu.h"
namespace po {
struct Edge { uint32_t u, v; int32_t weight, overlap_len; };
constexpr unsigned long long NODE_NO_RANK = ~0ull;
}
#include "../phasm_amd/csrc/merge.hip.h"
#include "../phasm_amd/csrc/components.hip.h"
using namespace po;
#include "rank_host_emu.h"

// what round_phase (components.hip.h) clears and reads back: the change words of one batch
struct EmuRounds {
    unsigned long long rcnt[CC_BATCH];
    uint64_t words[CC_BATCH];
    bool begin(uint32_t batch) {
        std::memset(rcnt, 0, sizeof rcnt);
        return batch > 0 && batch <= CC_BATCH;
    }
    bool end(uint32_t batch, const volatile uint64_t*& out) {
        for (uint32_t j = 0; j < CC_BATCH; ++j) words[j] = j < batch ? rcnt[j] : 0xDEADu;
        out = words;
        return true;
    }
};

int main() {
    RankedInput g;
    std::vector<uint32_t> p;
    const int status = ranked_input(g, p);
    if (status >= 0) return status;
    const uint32_t n = g.n, n_order = g.n_order, nn = g.nn;
    std::vector<uint32_t> comp(nn, 0xDEADu), ecomp(n + 1, 0xDEADu);
    std::vector<Component> table(nn, Component{0xDEADu, 0xDEADu, 0xDEADull});
    uint32_t rounds = 0, batches = 0;
    if (n_order) {
        EmuRounds ops;
        uint64_t lowered = 0;
        const int how = round_phase(ops, n_order, [&](uint32_t j) {
            if (n) LAUNCH(3, 4, k_cc_hook(g.ends.data(), n, n_order, p.data(), ops.rcnt + j));
            LAUNCH(3, 4, k_cc_jump(n_order, p.data(), ops.rcnt + j));
        }, rounds, batches, lowered);
        if (how != ROUNDS_DONE) { printf("cap\n"); return 0; }
        LAUNCH(3, 4, k_cc_roots(p.data(), n_order, g.root.data()));
    }
    const uint32_t n_comp = number_roots(g);
    if (n_comp) {
        std::memset(table.data(), 0, (size_t)n_comp * sizeof(Component));
        LAUNCH(3, 4, k_cc_label_nodes(p.data(), g.index.data(), g.val.data(), n_order, n_comp, comp.data(), table.data()));
        if (n) LAUNCH(3, 4, k_cc_label_edges(g.ends.data(), n, n_order, n_comp, comp.data(), ecomp.data(), table.data()));
        LAUNCH(3, 4, k_cc_max(table.data(), n_comp, g.cnt));
    }
    printf("%u %u %llu %llu %llu %u %u %llu\n", n_order, n_comp, g.cnt[KC_SINGLE], g.cnt[KC_MAXN], g.cnt[KC_MAXE], rounds, batches,
           (unsigned long long)cc_round_cap(n_order));
    for (uint32_t r = 0; r < n_order; ++r) printf("%u ", comp[r]);
    printf("\n");
    for (uint32_t i = 0; i < n; ++i) printf("%u ", ecomp[i]);
    printf("\n");
    for (uint32_t c = 0; c < n_comp; ++c) printf("%u %u %llu;", table[c].first_node, table[c].n_nodes, table[c].n_edges);
    printf("\n");
    return 0;
}
