// Host emulation of phasm_amd/csrc/superbubbles.hip.h for tests/test_superbubbles_host_emulation.py: the kernels compiled as
// plain C++ with ONE lane per wave (threads run one after another), so a machine without a GPU checks their indexing and
// logic -- behind the ranks and the SCC stage (the kernels of components.hip.h and partition.hip.h, as run_superbubbles of
// c_api.hip launches them through scc_stage): the degrees and the lists of D, sources and sinks, the level rounds, the two
// trees level by level, the pairs, the enclosing bubbles, the discards, the labels, the sums and the table -- against the
// goldens, under the host sanitizers.  The launches follow run_superbubbles: the same memsets, the same bounds, the batches
// and the stop at the first round that changes nothing from round_phase of components.hip.h, which run_superbubbles itself
// launches by.  The workspaces start as a call before could have left them.  Every loop here and in the kernels is bounded
// by a count.
//   stdin:  n_total n_edges n_order, one "u v" line per edge, the nodes in node order
//   stdout: "invalid N" alone, "bound WHAT" alone, or: order, SCCs, singletons, nodes and edges of P, bubbles, nested,
//           self-loop nodes, discarded, levels forward and backward; level rounds, discard rounds, batches, the largest
//           batch, the largest number of rounds a phase was given beyond its live nodes, launches per level in all; the exit
//           of every rank; the inside of every rank; the flags of every rank; per bubble "entrance exit n_inside nested;"
#include "host_emu.h"
namespace po {
struct Edge { uint32_t u, v; int32_t weight, overlap_len; };
constexpr unsigned long long NODE_NO_RANK = ~0ull;
}
#include "../phasm_amd/csrc/merge.hip.h"
#include "../phasm_amd/csrc/components.hip.h"
#include "../phasm_amd/csrc/partition.hip.h"
#include "../phasm_amd/csrc/superbubbles.hip.h"
using namespace po;

#include "rank_host_emu.h"

struct Batches {
    unsigned long long rcnt[CC_BATCH];
    uint64_t words[CC_BATCH];
    uint32_t max_batch = 0, in_batch = 0, batches = 0;
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
    void note(uint32_t j) {
        if (j != in_batch) in_batch = CC_BATCH + 1;
        ++in_batch;
    }
};

struct SccEmu : Batches {
    uint32_t n, n_order;
    const EdgeRanks* ends;
    uint8_t *live, *mark, *has_in, *has_out;
    uint32_t *scc, *colour;
    void trim_round(uint32_t j) {
        note(j);
        if (n) LAUNCH(3, 4, k_scc_trim_edges(ends, n, n_order, live, has_in, has_out));
        LAUNCH(3, 4, k_scc_trim_ranks(n_order, live, scc, has_in, has_out, rcnt + j));
    }
    void colour_init() { LAUNCH(3, 4, k_scc_colour_init(n_order, live, colour, mark)); }
    void forward_round(uint32_t j) {
        note(j);
        if (n) LAUNCH(3, 4, k_scc_forward(ends, n, n_order, live, colour, rcnt + j));
    }
    void back_init() { LAUNCH(3, 4, k_scc_back_init(n_order, live, colour, mark)); }
    void backward_round(uint32_t j) {
        note(j);
        if (n) LAUNCH(3, 4, k_scc_backward(ends, n, n_order, live, colour, mark, rcnt + j));
    }
    bool retire(uint64_t& retired) {
        unsigned long long c = 0;
        LAUNCH(3, 4, k_scc_retire(n_order, live, colour, mark, scc, &c));
        retired = c;
        return true;
    }
};

static void scan(const std::vector<uint32_t>& in, uint32_t n, std::vector<uint32_t>& out, uint64_t& total) {   // the library's prefix_sum
    total = 0;
    for (uint32_t r = 0; r < n; ++r) { out[r] = (uint32_t)total; total += in[r]; }
}

int main() {
    RankedInput g;
    std::vector<uint32_t> colour;
    const int status = ranked_input(g, colour);
    if (status >= 0) return status;
    const uint32_t n = g.n, n_order = g.n_order, nn = g.nn;
    const std::vector<EdgeRanks>& ends = g.ends;
    // ---- the SCC stage, as scc_stage launches it
    std::vector<uint32_t> scc(nn, 0xDEADu), node_scc(nn, 0xDEADu), flagw(nn, 0xDEADu);
    std::vector<uint8_t> live(nn, 9), mark(nn, 9), has_in(nn, 9), has_out(nn, 9), pflags(nn, 9), eclass(n + 1, 9);
    std::vector<Scc> sccs(nn, Scc{0xDEADu, 0xDEADu, 0xDEADull, 0xDEADu, 0xDEADu});
    SccWork W;
    if (n_order) {
        SccEmu ops;
        ops.n = n; ops.n_order = n_order; ops.ends = ends.data(); ops.live = live.data(); ops.mark = mark.data();
        ops.has_in = has_in.data(); ops.has_out = has_out.data(); ops.scc = scc.data(); ops.colour = colour.data();
        LAUNCH(3, 4, k_scc_init(n_order, live.data(), scc.data(), has_in.data(), has_out.data()));
        if (scc_drive(ops, n_order, W) != SCC_DONE) { printf("bound scc\n"); return 0; }
        LAUNCH(3, 4, k_scc_roots(scc.data(), n_order, g.root.data(), flagw.data()));
    }
    const uint32_t n_scc = number_roots(g);
    if (n_scc) {
        std::memset(sccs.data(), 0, (size_t)n_scc * sizeof(Scc));
        LAUNCH(3, 4, k_scc_label_nodes(scc.data(), g.index.data(), g.val.data(), n_order, n_scc, node_scc.data(), sccs.data()));
        if (n) LAUNCH(3, 4, k_scc_edges(ends.data(), n, n_order, n_scc, node_scc.data(), sccs.data(), eclass.data(), flagw.data(), g.cnt));
        LAUNCH(3, 4, k_scc_flags(n_order, n_scc, node_scc.data(), flagw.data(), sccs.data(), pflags.data()));
        LAUNCH(3, 4, k_scc_max(sccs.data(), n_scc, g.cnt));
    }
    if (!n_order) { printf("0 0 0 0 0 0 0 0 0 0 0\n0 0 0 0 0 0\n\n\n\n\n"); return 0; }
    // ---- the superbubbles, as run_superbubbles launches them
    std::vector<uint32_t> w(nn, 0xDEADu), cin(nn, 0xDEADu), cout(nn, 0xDEADu), off_in(nn, 0xDEADu), off_out(nn, 0xDEADu), cur_in(nn, 0xDEADu),
        cur_out(nn, 0xDEADu), list_in(n + 1, 0xDEADu), list_out(n + 1, 0xDEADu), lvl_f(nn, 0xDEADu), lvl_b(nn, 0xDEADu), idom(nn, 0xDEADu),
        ipdom(nn, 0xDEADu), depth(nn, 0xDEADu), exit_of(nn, 0xDEADu), encl(nn, 0xDEADu), inside(nn, 0xDEADu), total(nn, 0xDEADu),
        d_exit(nn, 0xDEADu), d_inside(nn, 0xDEADu);
    std::vector<uint8_t> dead(nn, 9), d_flags(nn, 9);
    std::vector<Bubble> table(nn, Bubble{0xDEADu, 0xDEADu, 0xDEADu, 0xDEADu});
    unsigned long long cnt[16] = {};
    LAUNCH(3, 4, k_sb_init(n_order, n_scc, node_scc.data(), sccs.data(), w.data(), cin.data(), cout.data(), idom.data(), ipdom.data(),
                           depth.data(), exit_of.data(), encl.data(), total.data(), dead.data()));
    if (n) LAUNCH(3, 4, k_sb_degrees(ends.data(), n, n_order, eclass.data(), w.data(), cin.data(), cout.data(), cnt));
    uint64_t sum_in = 0, sum_out = 0;
    scan(cin, n_order, off_in, sum_in);
    scan(cout, n_order, off_out, sum_out);
    std::fill(cur_in.begin(), cur_in.begin() + n_order, 0u);
    std::fill(cur_out.begin(), cur_out.begin() + n_order, 0u);
    if (n)
        LAUNCH(3, 4, k_sb_fill(ends.data(), n, n_order, eclass.data(), cin.data(), cout.data(), off_in.data(), off_out.data(), cur_in.data(),
                               cur_out.data(), list_in.data(), list_out.data()));
    LAUNCH(3, 4, k_sb_nodes(n_order, pflags.data(), cin.data(), cout.data(), w.data(), lvl_f.data(), lvl_b.data(), cnt));
    const uint64_t n_real = cnt[BC_REAL], n_dedges = cnt[BC_DEDGES];
    if (sum_in != n_dedges || sum_out != n_dedges || n_dedges > n || n_real > n_order) { printf("bound degrees\n"); return 0; }
    Batches ops;
    uint32_t level_rounds = 0, discard_rounds = 0;
    uint64_t ignored = 0, beyond = 0;
    int how = round_phase(ops, n_real, [&](uint32_t j) {
        ops.note(j);
        if (n) LAUNCH(3, 4, k_sb_level(ends.data(), n, n_order, eclass.data(), lvl_f.data(), lvl_b.data(), ops.rcnt + j));
    }, level_rounds, ops.batches, ignored);
    if (how != ROUNDS_DONE) { printf("bound levels\n"); return 0; }
    if (level_rounds > n_real) beyond = level_rounds - n_real;
    LAUNCH(3, 4, k_sb_level_max(n_order, lvl_f.data(), lvl_b.data(), cnt));
    const uint64_t levels_f = cnt[BC_LEVF], levels_b = cnt[BC_LEVB];
    if (levels_f > n_real || levels_b > n_real) { printf("bound level count\n"); return 0; }
    uint64_t per_level = 0;
    for (uint32_t l = 1; l <= levels_f; ++l, ++per_level)
        LAUNCH(3, 4, k_sb_tree(n_order, n, l, lvl_f.data(), off_in.data(), cin.data(), list_in.data(), w.data(), (uint32_t)SBW_SOURCE, idom.data(),
                               depth.data(), cnt));
    for (uint32_t l = 1; l <= levels_b; ++l, ++per_level)
        LAUNCH(3, 4, k_sb_tree(n_order, n, l, lvl_b.data(), off_out.data(), cout.data(), list_out.data(), w.data(), (uint32_t)SBW_SINK, ipdom.data(),
                               depth.data(), cnt));
    LAUNCH(3, 4, k_sb_pairs(n_order, w.data(), idom.data(), ipdom.data(), exit_of.data()));
    for (uint32_t l = 1; l <= levels_f; ++l, ++per_level)
        LAUNCH(3, 4, k_sb_encl(n_order, l, lvl_f.data(), idom.data(), exit_of.data(), encl.data()));
    if (cnt[BC_LOOPS]) {
        LAUNCH(3, 4, k_sb_dead_init(n_order, w.data(), idom.data(), exit_of.data(), encl.data(), dead.data()));
        how = round_phase(ops, n_real, [&](uint32_t j) {
            ops.note(j);
            LAUNCH(3, 4, k_sb_dead_round(n_order, exit_of.data(), encl.data(), dead.data(), ops.rcnt + j));
        }, discard_rounds, ops.batches, ignored);
        if (how != ROUNDS_DONE) { printf("bound discards\n"); return 0; }
        if (discard_rounds > n_real) beyond = std::max<uint64_t>(beyond, discard_rounds - n_real);
    }
    LAUNCH(3, 4, k_sb_label(n_order, g.val.data(), w.data(), idom.data(), exit_of.data(), encl.data(), dead.data(), inside.data(), total.data(),
                            g.root.data(), d_exit.data(), d_inside.data(), d_flags.data(), cnt));
    const uint32_t n_bubbles = number_roots(g);
    if (cnt[BC_WALK]) { printf("bound walk\n"); return 0; }
    if (n_bubbles > n_real || cnt[BC_NESTED] > n_bubbles) { printf("bound bubbles\n"); return 0; }
    if (cnt[BC_NESTED])
        for (uint32_t l = (uint32_t)levels_f; l >= 1; --l, ++per_level)
            LAUNCH(3, 4, k_sb_sum(n_order, l, lvl_f.data(), g.root.data(), inside.data(), total.data()));
    if (n_bubbles)
        LAUNCH(3, 4, k_sb_table(n_order, n_bubbles, g.val.data(), g.root.data(), g.index.data(), exit_of.data(), inside.data(), total.data(),
                                table.data()));
    printf("%u %u %llu %llu %llu %u %llu %llu %llu %llu %llu\n", n_order, n_scc, (unsigned long long)n_real,
           (unsigned long long)(n_real + (cnt[BC_R_EDGES] != 0) + (cnt[BC_RE_EDGES] != 0)),
           (unsigned long long)(n_dedges + cnt[BC_LOOPS] + cnt[BC_R_EDGES] + cnt[BC_RE_EDGES]), n_bubbles, cnt[BC_NESTED], cnt[BC_LOOPS],
           cnt[BC_DISCARDED], (unsigned long long)levels_f, (unsigned long long)levels_b);
    printf("%u %u %u %u %llu %llu\n", level_rounds, discard_rounds, ops.batches, ops.max_batch, (unsigned long long)beyond,
           (unsigned long long)per_level);
    for (uint32_t r = 0; r < n_order; ++r) printf("%u ", d_exit[r]);
    printf("\n");
    for (uint32_t r = 0; r < n_order; ++r) printf("%u ", d_inside[r]);
    printf("\n");
    for (uint32_t r = 0; r < n_order; ++r) printf("%u ", d_flags[r]);
    printf("\n");
    for (uint32_t i = 0; i < n_bubbles; ++i) printf("%u %u %u %u;", table[i].entrance, table[i].exit, table[i].n_inside, table[i].nested);
    printf("\n");
    return 0;
}
