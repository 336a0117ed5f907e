// Host emulation of phasm_amd/csrc/paths.hip.h for tests/test_paths_host_emulation.py: the kernels compiled as plain C++ with
// ONE lane per wave (threads run one after another), so a machine without a GPU checks their indexing and logic -- behind the
// ranks, the SCC stage, the superbubble stage (superbubble_stage_host_emu.h) and the bubble-chain stage with min_nodes = 1 (the
// kernels of bubblechains.hip.h, as bubblechains_host_emu.cpp launches them): the bubbles numbered by (chain, position), the
// two sorted key arrays of the edges and their segments, the counting rounds with the host's cap and batches, the table, the
// three offset arrays, the predecessors, the interior, and both passes of the walk of every listed path -- against the
// goldens, under the host sanitizers.
// The launches follow run_paths of c_api.hip: the same memsets, the same bounds, the same checks between them.  The
// workspaces start as a call before could have left them.  Every loop here and in the kernels is bounded by a count.
//   argv:   max_paths (decimal, up to 2^64 - 1; default 0)
//   stdin:  n_total n_edges n_order, one "u v weight" line per edge, the nodes in node order
//   stdout: "invalid N" alone, "bound WHAT" alone, "capacity WHAT" alone, or: bubbles, stray edges, bare, unlisted, saturated,
//           listed paths, path nodes, the greatest count, the longest path, counting rounds, batches, the largest batch;
//           per bubble "entrance exit chain position n_inside flags n_paths n_path_nodes;"; then one line each:
//           inside_off, inside_nodes, pred_off, pred_node, pred_weight, bubble_path_off, path_off, path_nodes
#include "host_emu.h"
#include <cstdlib>
namespace po {
struct Edge { uint32_t u, v; int32_t weight, overlap_len; };
constexpr unsigned long long NODE_NO_RANK = ~0ull;
}
#include "../phasm_amd/csrc/merge.hip.h"
#include "../phasm_amd/csrc/components.hip.h"
#include "../phasm_amd/csrc/partition.hip.h"
#include "../phasm_amd/csrc/superbubbles.hip.h"
#include "../phasm_amd/csrc/bubblechains.hip.h"
#include "../phasm_amd/csrc/paths.hip.h"
using namespace po;

#include "rank_host_emu.h"
#include "superbubble_stage_host_emu.h"

template <class T>
static void line(const std::vector<T>& v, size_t n) {
    for (size_t i = 0; i < n; ++i) printf("%lld ", (long long)v[i]);
    printf("\n");
}

int main(int argc, char** argv) {
    const unsigned long long max_paths = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 0ull;
    RankedInput g;
    std::vector<uint32_t> colour;
    const int status = ranked_input(g, colour, true);
    if (status >= 0) return status;
    const uint32_t n = g.n, n_order = g.n_order, nn = g.nn;
    const std::vector<EdgeRanks>& ends = g.ends;
    SuperbubbleStage S;
    if (!S.run(g, colour)) return 0;
    const char* const nothing = "0 0 0 0 0 0 0 0 0 0 0 0\n\n0 \n\n0 \n\n\n0 \n0 \n\n";
    if (!n_order) { printf("%s", nothing); return 0; }
    const uint32_t n_bubbles_all = S.n_bubbles;
    const uint64_t n_nested = S.cnt[BC_NESTED];
    uint64_t ignored = 0;
    int how;
    // ---- the bubble chains with min_nodes = 1, as bubblechain_stage launches them
    std::vector<uint32_t> fw(nn, 0xDEADu), next(nn, 0xDEADu), pred(nn, 0xDEADu), top(nn, 0xDEADu), jb0(nn, 0xDEADu), jb1(nn, 0xDEADu),
        hops0(nn, 0xDEADu), hops1(nn, 0xDEADu), nhead(nn, 0xDEADu), npos(nn, 0xDEADu), cb(nn, 0xDEADu), cn(nn, 0xDEADu), last(nn, 0xDEADu),
        d_chain(nn, 0xDEADu), d_bubble(nn, 0xDEADu);
    std::vector<unsigned long long> ce(nn, 0xDEADull);
    std::vector<BubbleChain> chains(nn, BubbleChain{0xDEADu, 0xDEADu, 0xDEADu, 0xDEADu, 0xDEADull});
    uint32_t* jb[2] = {jb0.data(), jb1.data()};
    uint32_t* hops[2] = {hops0.data(), hops1.data()};
    unsigned long long hc[16] = {};
    LAUNCH(3, 4, k_bc_init(n_order, g.root.data(), S.inside.data(), fw.data(), next.data(), pred.data(), top.data(), cb.data(), cn.data(),
                           ce.data(), last.data()));
    LAUNCH(3, 4, k_bc_link(n_order, fw.data(), S.exit_of.data(), next.data(), pred.data(), hc));
    LAUNCH(3, 4, k_bc_heads(n_order, pred.data(), fw.data(), jb[0], hops[0], hc));
    const uint64_t n_top = hc[HK_TOP], n_heads = hc[HK_HEADS];
    if (n_top + n_nested != n_bubbles_all || n_heads > n_top || (n_top && !n_heads)) { printf("bound top\n"); return 0; }
    Batches bops;
    uint32_t nest_rounds = 0, chain_rounds = 0;
    if (n_top && n_nested) {
        how = round_phase(bops, n_nested, [&](uint32_t j) {
            bops.note(j);
            LAUNCH(3, 4, k_bc_nest(n_order, top.data(), bops.rcnt + j));
        }, nest_rounds, bops.batches, ignored);
        if (how != ROUNDS_DONE) { printf("bound holders\n"); return 0; }
    }
    uint32_t launched = 0;
    if (n_top) {
        how = round_phase(bops, n_top, [&](uint32_t j) {
            bops.note(j);
            const uint32_t a = launched & 1, b = a ^ 1;
            LAUNCH(3, 4, k_bc_jump(n_order, jb[a], hops[a], jb[b], hops[b], bops.rcnt + j));
            ++launched;
        }, chain_rounds, bops.batches, ignored);
        if (how != ROUNDS_DONE) { printf("bound ranking\n"); return 0; }
    }
    const uint32_t fin = launched & 1;
    LAUNCH(3, 4, k_bc_place(n_order, fw.data(), next.data(), pred.data(), top.data(), S.exit_of.data(), jb[fin], hops[fin], nhead.data(),
                            npos.data(), cb.data(), cn.data(), last.data(), hc));
    if (n) LAUNCH(3, 4, k_bc_edges(ends.data(), n, n_order, nhead.data(), ce.data()));
    LAUNCH(3, 4, k_bc_filter(n_order, 1u, fw.data(), cb.data(), cn.data(), ce.data(), g.root.data(), hc));
    const uint32_t n_chains = number_roots(g);
    if (hc[HK_BAD]) { printf("bound head\n"); return 0; }
    if (n_chains != hc[HK_CHAINS] || n_chains + hc[HK_SHORT] != n_heads) { printf("bound chains\n"); return 0; }
    if (n_chains)
        LAUNCH(3, 4, k_bc_table(n_order, n_chains, g.val.data(), g.root.data(), g.index.data(), last.data(), cb.data(), cn.data(), ce.data(),
                                chains.data()));
    LAUNCH(3, 4, k_bc_nodes(n_order, n_chains, g.root.data(), g.index.data(), nhead.data(), npos.data(), d_chain.data(), d_bubble.data()));
    // ---- the paths, as run_paths launches them
    const uint32_t n_b = (uint32_t)n_top;
    if (!n_b) { printf("%s", nothing); return 0; }
    if (!n) { printf("bound edges\n"); return 0; }
    const uint32_t pad_n = merge_sort_pad(n), pad_o = merge_sort_pad(n_order);
    std::vector<uint32_t> nb(nn, 0xDEADu), coff(nn, 0xDEADu), home(nn, 0xDEADu), bidx(nn, 0xDEADu), bent(nn, 0xDEADu), done(nn, 0xDEADu),
        ofirst(nn, 0xDEADu), olast(nn, 0xDEADu), ifirst(nn, 0xDEADu), ilast(nn, 0xDEADu), n_list(nn, 0xDEADu), n_pred(nn, 0xDEADu),
        n_in(nn, 0xDEADu), in_off(n_b + 1, 0xDEADu), pred_off(n_b + 1, 0xDEADu), bpo(n_b + 1, 0xDEADu);
    std::vector<unsigned long long> count(nn, 0xDEADull), key_out(pad_n, 7), key_in(pad_n, 7), key_inside(pad_o, 7);
    std::vector<BubblePaths> table(n_b, BubblePaths{0xDEADu, 0xDEADu, 0xDEADu, 0xDEADu, 0xDEADu, 0xDEADu, 0xDEADull, 0xDEADull});
    unsigned long long pc[16] = {};
    uint64_t total = 0;
    auto sort_keys = [&](std::vector<unsigned long long>& key, uint32_t items, uint32_t pad) {
        merge_sort_steps(items, [&](uint32_t j, uint32_t k) { LAUNCH(3, 4, k_pp_bitonic(key.data(), pad, j, k)); });
    };
    LAUNCH(3, 4, k_pp_chain_counts(n_chains, chains.data(), nb.data()));
    scan(nb, n_chains + 1, coff, total);
    const uint64_t numbered = total;
    std::fill(bent.begin(), bent.begin() + n_order, 0xFFFFFFFFu);
    for (auto* v : {&ofirst, &olast, &ifirst, &ilast}) std::fill(v->begin(), v->begin() + n_order, 0u);
    LAUNCH(3, 4, k_pp_bubbles(n_order, n_chains, n_b, fw.data(), top.data(), d_chain.data(), d_bubble.data(), coff.data(), S.total.data(),
                              home.data(), bidx.data(), bent.data(), done.data(), count.data(), pc));
    LAUNCH(3, 4, k_pp_keys(ends.data(), n, n_order, pad_n, home.data(), S.exit_of.data(), pred.data(), key_out.data(), key_in.data(), pc));
    sort_keys(key_out, n, pad_n);
    sort_keys(key_in, n, pad_n);
    LAUNCH(3, 4, k_pp_segments(key_out.data(), n, n_order, ofirst.data(), olast.data()));
    LAUNCH(3, 4, k_pp_segments(key_in.data(), n, n_order, ifirst.data(), ilast.data()));
    if (numbered != n_b || pc[QK_BAD] || pc[QK_MAXIN] > n_order) { printf("bound bubbles\n"); return 0; }
    const uint64_t max_inside = pc[QK_MAXIN];
    uint32_t count_rounds = 0, launch = 0;
    Batches cops;
    how = round_phase(cops, max_inside, [&](uint32_t j) {
        cops.note(j);
        ++launch;
        LAUNCH(3, 4, k_pp_count(n_order, n, launch, home.data(), S.exit_of.data(), ofirst.data(), olast.data(), key_out.data(), ends.data(),
                                done.data(), count.data(), cops.rcnt + j));
    }, count_rounds, cops.batches, ignored);
    if (how != ROUNDS_DONE) { printf("bound counts\n"); return 0; }
    LAUNCH(3, 4, k_pp_table(n_b, n_order, max_paths, bent.data(), S.exit_of.data(), g.val.data(), d_chain.data(), d_bubble.data(), S.total.data(),
                            count.data(), ifirst.data(), ilast.data(), table.data(), n_list.data(), n_pred.data(), n_in.data(), pc));
    uint64_t listed_total = 0, preds64 = 0, inside64 = 0;
    scan(n_list, n_b + 1, bpo, listed_total);
    scan(n_pred, n_b + 1, pred_off, preds64);
    scan(n_in, n_b + 1, in_off, inside64);
    const uint64_t listed64 = pc[QK_LISTED];
    if (listed64 >= (1ull << 30)) { printf("capacity paths\n"); return 0; }
    if (listed_total != listed64 || preds64 > n || inside64 > n_order) { printf("bound offsets\n"); return 0; }
    const uint32_t n_listed = (uint32_t)listed64, n_preds = (uint32_t)preds64, n_inside = (uint32_t)inside64;
    std::vector<uint32_t> plen(n_listed + 1, 0xDEADu), poff(n_listed + 1, 0xDEADu), pred_node(n_preds, 0xDEADu), inside_nodes(n_inside, 0xDEADu);
    std::vector<int32_t> pred_weight(n_preds, 0xDEAD);
    LAUNCH(3, 4, k_pp_preds(n, n_order, n_preds, key_in.data(), ends.data(), g.e.data(), pred.data(), bidx.data(), ifirst.data(),
                            pred_off.data(), g.val.data(), pred_node.data(), pred_weight.data(), pc));
    LAUNCH(3, 4, k_pp_inside_keys(n_order, pad_o, home.data(), bidx.data(), key_inside.data(), pc));
    sort_keys(key_inside, n_order, pad_o);
    if (n_inside) LAUNCH(3, 4, k_pp_inside(n_inside, n_order, key_inside.data(), g.val.data(), inside_nodes.data()));
    LAUNCH(3, 4, k_pp_walk<false>(n_listed, n_b, n_order, n, 0u, bpo.data(), bent.data(), S.exit_of.data(), S.total.data(), home.data(),
                                  ofirst.data(), olast.data(), key_out.data(), ends.data(), count.data(), g.val.data(), plen.data(),
                                  (const uint32_t*)nullptr, (uint32_t*)nullptr, pc));
    uint64_t nodes64 = 0;
    scan(plen, n_listed + 1, poff, nodes64);
    if (pc[QK_BAD] || pc[QK_INSIDE] != n_inside) { printf("bound interior\n"); return 0; }
    if (pc[QK_WALK]) { printf("bound walk\n"); return 0; }
    if (nodes64 >= (1ull << 31)) { printf("capacity nodes\n"); return 0; }
    if (nodes64 < 2 * listed64 || pc[QK_MAXLEN] > max_inside + 2) { printf("bound lengths\n"); return 0; }
    const uint32_t n_path_nodes = (uint32_t)nodes64;
    std::vector<uint32_t> path_nodes(n_path_nodes, 0xDEADu);
    if (n_listed)
        LAUNCH(3, 4, k_pp_walk<true>(n_listed, n_b, n_order, n, n_path_nodes, bpo.data(), bent.data(), S.exit_of.data(), S.total.data(),
                                     home.data(), ofirst.data(), olast.data(), key_out.data(), ends.data(), count.data(), g.val.data(),
                                     (uint32_t*)nullptr, poff.data(), path_nodes.data(), pc));
    LAUNCH(3, 4, k_pp_bubble_nodes(n_b, bpo.data(), poff.data(), table.data()));
    if (pc[QK_WALK]) { printf("bound rows\n"); return 0; }
    printf("%u %llu %llu %llu %llu %u %u %llu %llu %u %u %u\n", n_b, pc[QK_STRAY], pc[QK_BARE], pc[QK_UNLISTED], pc[QK_SATURATED], n_listed,
           n_path_nodes, pc[QK_MAXPATHS], pc[QK_MAXLEN], count_rounds, cops.batches, cops.max_batch);
    for (uint32_t b = 0; b < n_b; ++b)
        printf("%u %u %u %u %u %u %llu %llu;", table[b].entrance, table[b].exit, table[b].chain, table[b].position, table[b].n_inside,
               table[b].flags, table[b].n_paths, table[b].n_path_nodes);
    printf("\n");
    line(in_off, n_b + 1);
    line(inside_nodes, n_inside);
    line(pred_off, n_b + 1);
    line(pred_node, n_preds);
    line(pred_weight, n_preds);
    line(bpo, n_b + 1);
    line(poff, n_listed + 1);
    line(path_nodes, n_path_nodes);
    return 0;
}
