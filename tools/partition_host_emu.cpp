// Host emulation of phasm_amd/csrc/partition.hip.h for tests/test_partition_host_emulation.py: the kernels compiled as plain
// C++ with ONE lane per wave (threads run one after another), so a machine without a GPU checks their indexing and logic
// -- the ranks (the kernels of components.hip.h, as po_layout_partition launches them), the trim rounds, the forward
// colouring, the backward marking, the retiring, the numbering of the roots, the table, the edge classes and the node flags
// -- against the goldens, under the host sanitizers.  The launches follow run_partition (c_api.hip): the same memsets, and
// every bound, the batches and the stop at the first round that changes nothing come from scc_drive of partition.hip.h
// and round_phase of components.hip.h, which run_partition itself launches by.  The workspaces start as a call before
// could have left them.  Every loop here and in the kernels is bounded by a count.
//   stdin:  n_total n_edges n_order, one "u v" line per edge, the nodes in node order (node ids < n_total; ids at or
//           above the reads are merged nodes: the kernels do not tell them apart)
//   stdout: "invalid N" alone, "bound K" alone, or: order, SCCs, singletons, max nodes, max edges, self-loops, the five class
//           counts; trimmed, iterations, trim / forward / backward rounds, batches, the largest batch, the largest number of
//           rounds one phase was given beyond its live nodes; the SCC of every rank; the flags of every rank; the class of
//           every edge; per SCC "first_node n_nodes n_edges n_r_in n_re_out;"
#include "host_emu.h"
namespace po {
struct Edge { uint32_t u, v; int32_t weight, overlap_len; };
constexpr unsigned long long NODE_NO_RANK = ~0ull;
}
#include "../phasm_amd/csrc/merge.hip.h"
#include "../phasm_amd/csrc/components.hip.h"
#include "../phasm_amd/csrc/partition.hip.h"
using namespace po;

#include "rank_host_emu.h"

struct EmuOps {
    uint32_t n, n_order;
    const EdgeRanks* ends;
    uint8_t *live, *mark, *has_in, *has_out;
    uint32_t *scc, *colour;
    unsigned long long rcnt[CC_BATCH];
    uint64_t words[CC_BATCH];
    uint32_t max_batch = 0, in_batch = 0, live_now = 0;
    uint64_t phase_rounds = 0, max_beyond_live = 0;
    bool begin(uint32_t batch) {
        if (batch == 0 || batch > CC_BATCH) return false;
        std::memset(rcnt, 0, sizeof rcnt);
        max_batch = std::max(max_batch, batch);
        in_batch = 0;
        return true;
    }
    bool end(uint32_t batch, const volatile uint64_t*& out) {
        if (in_batch != batch) return false;   // (every round of the batch was launched, and no more)
        for (uint32_t j = 0; j < CC_BATCH; ++j) words[j] = j < batch ? rcnt[j] : 0xDEADu;
        out = words;
        return true;
    }
    void count_live() {
        live_now = 0;
        for (uint32_t r = 0; r < n_order; ++r) live_now += live[r];
    }
    void note(uint32_t j) {   // a round may only ever be launched while the phase is within its live nodes + 2
        if (j != in_batch) in_batch = CC_BATCH + 1;
        ++in_batch;
        ++phase_rounds;
    }
    void phase_start() {
        count_live();
        phase_rounds = 0;
    }
    void phase_end() { if (phase_rounds > live_now) max_beyond_live = std::max<uint64_t>(max_beyond_live, phase_rounds - live_now); }
    bool trim_started = false, fwd_started = false, bwd_started = false;
    void trim_round(uint32_t j) {
        if (!trim_started) { phase_start(); trim_started = true; }
        note(j);
        if (n) LAUNCH(3, 4, k_scc_trim_edges(ends, n, n_order, live, has_in, has_out));
        LAUNCH(3, 4, k_scc_trim_ranks(n_order, live, scc, has_in, has_out, rcnt + j));
    }
    void colour_init() {
        phase_end();
        trim_started = false;
        LAUNCH(3, 4, k_scc_colour_init(n_order, live, colour, mark));
    }
    void forward_round(uint32_t j) {
        if (!fwd_started) { phase_start(); fwd_started = true; }
        note(j);
        if (n) LAUNCH(3, 4, k_scc_forward(ends, n, n_order, live, colour, rcnt + j));
    }
    void back_init() {
        phase_end();
        fwd_started = false;
        LAUNCH(3, 4, k_scc_back_init(n_order, live, colour, mark));
    }
    void backward_round(uint32_t j) {
        if (!bwd_started) { phase_start(); bwd_started = true; }
        note(j);
        if (n) LAUNCH(3, 4, k_scc_backward(ends, n, n_order, live, colour, mark, rcnt + j));
    }
    bool retire(uint64_t& retired) {
        phase_end();
        bwd_started = false;
        unsigned long long c = 0;
        LAUNCH(3, 4, k_scc_retire(n_order, live, colour, mark, scc, &c));
        retired = c;
        return true;
    }
};

int main() {
    RankedInput g;
    std::vector<uint32_t> colour;
    const int status = ranked_input(g, colour);
    if (status >= 0) return status;
    const uint32_t n = g.n, n_order = g.n_order, nn = g.nn;
    const std::vector<EdgeRanks>& ends = g.ends;
    std::vector<uint32_t> scc(nn, 0xDEADu), node_scc(nn, 0xDEADu), flagw(nn, 0xDEADu);
    std::vector<uint8_t> live(nn, 9), mark(nn, 9), has_in(nn, 9), has_out(nn, 9), flags(nn, 9), eclass(n + 1, 9);
    std::vector<Scc> table(nn, Scc{0xDEADu, 0xDEADu, 0xDEADull, 0xDEADu, 0xDEADu});
    unsigned long long* cnt = g.cnt;
    SccWork W;
    EmuOps ops{n, n_order, ends.data(), live.data(), mark.data(), has_in.data(), has_out.data(), scc.data(), colour.data(), {}, {}};
    if (n_order) {
        LAUNCH(3, 4, k_scc_init(n_order, live.data(), scc.data(), has_in.data(), has_out.data()));
        const int how = scc_drive(ops, n_order, W);
        if (how != SCC_DONE) { printf("bound %d\n", how); return 0; }
        ops.phase_end();
        for (uint32_t r = 0; r < n_order; ++r) if (live[r] || scc[r] > r) { printf("live\n"); return 0; }
        LAUNCH(3, 4, k_scc_roots(scc.data(), n_order, g.root.data(), flagw.data()));
    }
    const uint32_t n_scc = number_roots(g);
    if (n_scc) {
        std::memset(table.data(), 0, (size_t)n_scc * sizeof(Scc));
        LAUNCH(3, 4, k_scc_label_nodes(scc.data(), g.index.data(), g.val.data(), n_order, n_scc, node_scc.data(), table.data()));
        if (n) LAUNCH(3, 4, k_scc_edges(ends.data(), n, n_order, n_scc, node_scc.data(), table.data(), eclass.data(), flagw.data(), cnt));
        LAUNCH(3, 4, k_scc_flags(n_order, n_scc, node_scc.data(), flagw.data(), table.data(), flags.data()));
        LAUNCH(3, 4, k_scc_max(table.data(), n_scc, cnt));
    }
    printf("%u %u %llu %llu %llu %llu %llu %llu %llu %llu %llu\n", n_order, n_scc, cnt[PC_SINGLE], cnt[PC_MAXN], cnt[PC_MAXE], cnt[PC_SELF],
           cnt[PC_CLASS], cnt[PC_CLASS + 1], cnt[PC_CLASS + 2], cnt[PC_CLASS + 3], cnt[PC_CLASS + 4]);
    printf("%llu %u %u %u %u %u %u %llu\n", (unsigned long long)W.n_trimmed, W.outer, W.trim_rounds, W.forward_rounds, W.backward_rounds,
           W.batches, ops.max_batch, (unsigned long long)ops.max_beyond_live);
    for (uint32_t r = 0; r < n_order; ++r) printf("%u ", node_scc[r]);
    printf("\n");
    for (uint32_t r = 0; r < n_order; ++r) printf("%u ", flags[r]);
    printf("\n");
    for (uint32_t i = 0; i < n; ++i) printf("%u ", eclass[i]);
    printf("\n");
    for (uint32_t c = 0; c < n_scc; ++c)
        printf("%u %u %llu %u %u;", table[c].first_node, table[c].n_nodes, table[c].n_edges, table[c].n_r_in, table[c].n_re_out);
    printf("\n");
    return 0;
}
