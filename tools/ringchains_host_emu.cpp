// Host emulation of phasm_amd/csrc/ringchains.hip.h for tests/test_bubblechains_all_host_emulation.py: the kernels of the ring
// election and the unchanged kernels of bubblechains.hip.h around them, compiled as plain C++ with ONE lane per wave (threads
// run one after another), so a machine without a GPU checks their indexing and logic under the host sanitizers.  The bubble
// source is GIVEN: the words that po_layout_superbubbles_all's stage leaves per original rank (the byte "enters a surviving
// bubble", exit_of, the holder) and its counts come in behind the graph, from phasm_amd.cyclic.HostSuperbubblesAll, which
// tests/test_cyclic_host_emulation.py holds equal to that stage's own emulation (tools/cyclic_host_emu.cpp).
// The launches follow bubblechain_stage of c_api.hip behind CyclicBubbles: the same memsets, the same bounds, the election's
// fixed number of rounds between its two buffer pairs, the batches and the stop at the first round that changes nothing from
// round_phase of components.hip.h.  The workspaces start as a call before could have left them.  Every loop here and in the
// kernels is bounded by a count.
//   argv:   min_nodes (default 1)
//   stdin:  n_total n_edges n_order, one "u v" line per edge, the nodes in node order; then "n_bubbles n_nested n_cyclic" and
//           per rank "enters exit_of inside" (ranks; 4294967295: none)
//   stdout: "invalid N" alone, "bound WHAT" alone, or: order, top-level bubbles, path heads, heads, chains, short chains, chain
//           nodes, chain edges, bubbles of the longest chain, ring chains, ring bubbles, election rounds; holder rounds,
//           ranking rounds, batches of the two loops, the largest batch; the chain of every rank; the position of every rank;
//           the chain of every edge (as given); per chain "first_entrance last_exit n_bubbles n_nodes n_edges;"
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
#include "../phasm_amd/csrc/ringchains.hip.h"
using namespace po;

#include "rank_host_emu.h"
#include "superbubble_stage_host_emu.h"   // (for Batches: what round_phase clears and reads back)

int main(int argc, char** argv) {
    const uint32_t min_nodes = argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 10) : 1u;
    RankedInput g;
    std::vector<uint32_t> ident;
    const int status = ranked_input(g, ident);
    if (status >= 0) return status;
    const uint32_t n = g.n, n_order = g.n_order, nn = g.nn;
    const std::vector<EdgeRanks>& ends = g.ends;
    unsigned long long n_bubbles = 0, n_nested = 0, n_cyclic = 0;
    if (scanf("%llu %llu %llu", &n_bubbles, &n_nested, &n_cyclic) != 3) return 1;
    std::vector<uint8_t> enters(nn, 9);
    std::vector<uint32_t> exit_of(nn, 0xDEADu), inside(nn, 0xDEADu);
    for (uint32_t r = 0; r < n_order; ++r) {
        uint32_t a, b, c;
        if (scanf("%u %u %u", &a, &b, &c) != 3) return 1;
        enters[r] = (uint8_t)a;
        exit_of[r] = b;
        inside[r] = c;
    }
    if (!n_order) { printf("0 0 0 0 0 0 0 0 0 0 0 0\n0 0 0 0\n\n\n\n\n"); return 0; }
    const bool rings = n_cyclic > 0;
    uint64_t ignored = 0;
    int how;
    // ---- the bubble chains, as bubblechain_stage launches them behind CyclicBubbles
    std::vector<uint32_t> fw(nn, 0xDEADu), next(nn, 0xDEADu), pred(nn, 0xDEADu), top(nn, 0xDEADu), jb0(nn, 0xDEADu), jb1(nn, 0xDEADu),
        hops0(nn, 0xDEADu), hops1(nn, 0xDEADu), nhead(nn, 0xDEADu), npos(nn, 0xDEADu), cb(nn, 0xDEADu), cn(nn, 0xDEADu), last(nn, 0xDEADu),
        d_chain(nn, 0xDEADu), d_bubble(nn, 0xDEADu), d_edge(n + 1, 0xDEADu), ptr0(nn, 0xDEADu), ptr1(nn, 0xDEADu), mn0(nn, 0xDEADu),
        mn1(nn, 0xDEADu);
    std::vector<unsigned long long> ce(nn, 0xDEADull);
    std::vector<BubbleChain> chains(nn, BubbleChain{0xDEADu, 0xDEADu, 0xDEADu, 0xDEADu, 0xDEADull});
    uint32_t* jb[2] = {jb0.data(), jb1.data()};
    uint32_t* hops[2] = {hops0.data(), hops1.data()};
    uint32_t* ptr[2] = {ptr0.data(), ptr1.data()};
    uint32_t* mn[2] = {mn0.data(), mn1.data()};
    unsigned long long hc[16] = {};
    LAUNCH(3, 4, k_bc_init(n_order, enters.data(), inside.data(), fw.data(), next.data(), pred.data(), top.data(), cb.data(), cn.data(),
                           ce.data(), last.data()));
    LAUNCH(3, 4, k_bc_link(n_order, fw.data(), exit_of.data(), next.data(), pred.data(), hc));
    LAUNCH(3, 4, k_bc_heads(n_order, pred.data(), fw.data(), jb[0], hops[0], hc));
    const uint64_t n_top = hc[HK_TOP], n_path_heads = hc[HK_HEADS];
    uint64_t n_heads = n_path_heads;
    if (n_top + n_nested != n_bubbles || n_heads > n_top || (n_top && !n_heads && !rings)) { printf("bound top\n"); return 0; }
    uint32_t ring_rounds_run = 0;
    uint64_t n_rings = 0;
    if (n_top && rings) {
        const uint32_t rounds = ring_rounds(n_top);
        LAUNCH(3, 4, k_rc_init(n_order, jb[0], ptr[0], mn[0]));
        for (uint32_t k = 0; k < rounds; ++k) LAUNCH(3, 4, k_rc_round(n_order, ptr[k & 1], mn[k & 1], ptr[(k & 1) ^ 1], mn[(k & 1) ^ 1]));
        LAUNCH(3, 4, k_rc_leaders(n_order, ptr[rounds & 1], mn[rounds & 1], fw.data(), jb[0], hops[0], hc));
        ring_rounds_run = rounds;
        n_rings = hc[HKR_RINGS];
        if (hc[HK_HEADS] != n_heads + n_rings || hc[HK_HEADS] > n_top || !hc[HK_HEADS]) { printf("bound leaders\n"); return 0; }
        n_heads = hc[HK_HEADS];
    }
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
    LAUNCH(3, 4, k_bc_place(n_order, fw.data(), next.data(), pred.data(), top.data(), exit_of.data(), jb[fin], hops[fin], nhead.data(),
                            npos.data(), cb.data(), cn.data(), last.data(), hc));
    if (n_rings) LAUNCH(3, 4, k_rc_close(n_order, fw.data(), cb.data(), last.data(), hc));
    if (n) LAUNCH(3, 4, k_bc_edges(ends.data(), n, n_order, nhead.data(), ce.data()));
    LAUNCH(3, 4, k_bc_filter(n_order, min_nodes, fw.data(), cb.data(), cn.data(), ce.data(), g.root.data(), hc));
    const uint32_t n_chains = number_roots(g);
    if (hc[HK_BAD]) { printf("bound head\n"); return 0; }
    if (n_chains != hc[HK_CHAINS] || n_chains + hc[HK_SHORT] != n_heads || hc[HK_CNODES] > n_order || hc[HK_CEDGES] > n || hc[HK_MAXB] > n_top) {
        printf("bound chains\n");
        return 0;
    }
    if (n_rings && (hc[HKR_RBUBBLES] < n_rings || hc[HKR_RBUBBLES] > n_top)) { printf("bound rings\n"); return 0; }
    if (n_chains)
        LAUNCH(3, 4, k_bc_table(n_order, n_chains, g.val.data(), g.root.data(), g.index.data(), last.data(), cb.data(), cn.data(), ce.data(),
                                chains.data()));
    LAUNCH(3, 4, k_bc_nodes(n_order, n_chains, g.root.data(), g.index.data(), nhead.data(), npos.data(), d_chain.data(), d_bubble.data()));
    if (n) LAUNCH(3, 4, k_bc_edge_out(ends.data(), n, n_order, d_chain.data(), d_edge.data()));
    printf("%u %llu %llu %llu %u %llu %llu %llu %llu %llu %llu %u\n", n_order, (unsigned long long)n_top, (unsigned long long)n_path_heads,
           (unsigned long long)n_heads, n_chains, hc[HK_SHORT], hc[HK_CNODES], hc[HK_CEDGES], hc[HK_MAXB], (unsigned long long)n_rings,
           hc[HKR_RBUBBLES], ring_rounds_run);
    printf("%u %u %u %u\n", nest_rounds, chain_rounds, bops.batches, bops.max_batch);
    for (uint32_t r = 0; r < n_order; ++r) printf("%u ", d_chain[r]);
    printf("\n");
    for (uint32_t r = 0; r < n_order; ++r) printf("%u ", d_bubble[r]);
    printf("\n");
    for (uint32_t e = 0; e < n; ++e) printf("%u ", d_edge[e]);
    printf("\n");
    for (uint32_t i = 0; i < n_chains; ++i)
        printf("%u %u %u %u %llu;", chains[i].first_entrance, chains[i].last_exit, chains[i].n_bubbles, chains[i].n_nodes, chains[i].n_edges);
    printf("\n");
    return 0;
}
