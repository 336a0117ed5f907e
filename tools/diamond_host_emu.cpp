// Host emulation of phasm_amd/csrc/diamond.hip.h for tests/test_diamond_host_emulation.py: the kernels compiled as plain
// C++ with ONE lane per wave (threads run one after another), so a machine without a GPU checks their indexing and
// logic -- degrees and in-edge ids, the footprints, the rounds, the node pass -- against the goldens, under the host
// sanitizers.  The candidate list is scrambled before the rounds: the answer must not depend on its order.  Threads of
// k_diamond_resolve run one after another, so a later thread sees the removals of an earlier one of the same round -- one
// of the interleavings the device may produce.  The mark words start all ones, as the call's memset leaves them, and
// after every k_diamond_mark each word an unresolved candidate is about to read must have been written ("unwritten").
//   stdin:  n_nodes n_edges n_order, then one "u v" line per edge, then the nodes in node order
//   stdout: the flag digits; the counters invalid, candidates, diamonds, nodes, removed, kept and the rounds; the nodes
//           left, in order
#include "host_emu.h"
namespace po {
struct Edge { uint32_t u, v; int32_t weight, overlap_len; };
constexpr unsigned long long EDGE_EMPTY = ~0ull;
static inline uint32_t edge_slot(uint32_t u, uint32_t v, uint32_t n_slots) {
    const unsigned long long k = (((unsigned long long)u << 32) | v) * 0x9E3779B97F4A7C15ull;
    return (uint32_t)(((k >> 32) * (unsigned long long)n_slots) >> 32);
}
}
#include "../phasm_amd/csrc/tips.hip.h"
#include "../phasm_amd/csrc/diamond.hip.h"
using namespace po;
int main() {
    uint32_t n_nodes, n, n_order;
    if (scanf("%u %u %u", &n_nodes, &n, &n_order) != 3) return 1;
    std::vector<Edge> e(n);
    for (uint32_t i = 0; i < n; ++i) { if (scanf("%u %u", &e[i].u, &e[i].v) != 2) return 1; e[i].weight = 500; e[i].overlap_len = 0; }
    std::vector<unsigned long long> nrank(n_nodes, NODE_NO_RANK), nrank_out(n_nodes, 7), mark(n_nodes, ~0ull);
    for (uint32_t i = 0; i < n_order; ++i) { uint32_t x; if (scanf("%u", &x) != 1 || x >= n_nodes) return 1; nrank[x] = ((unsigned long long)(3u * i + 5) << 2) | (i & 3); }
    std::vector<uint32_t> outdeg(n_nodes, 0), indeg(n_nodes, 0), inmin(n_nodes, 0xFFFFFFFFu), inmax(n_nodes, 0), cand(n_nodes + 1, 0xDEADu);
    // (the other workspaces start as a call before could have left them)
    std::vector<uint8_t> cstate(n_nodes + 1, 9), removed(n_nodes + 1, 9), eflag(n + 1, 9), keep(n + 1, 9);
    unsigned long long cnt[16] = {};
    LAUNCH(3, 4, k_diamond_degree(e.data(), n, n_nodes, outdeg.data(), indeg.data(), inmin.data(), inmax.data(), eflag.data(), cnt));
    LAUNCH((n_nodes + 3) / 4, 4, k_diamond_candidates(n_nodes, nrank.data(), outdeg.data(), indeg.data(), cand.data(), cstate.data(), removed.data(), cnt));
    if (cnt[DC_INVALID]) { printf("invalid\n"); return 0; }
    const uint32_t n_cand = (uint32_t)cnt[DC_CAND];
    std::vector<uint32_t> scr(n_cand);
    for (uint32_t t = 0; t < n_cand; ++t) scr[t] = cand[n_cand % 7919u == 0 ? t : (uint32_t)(((uint64_t)t * 7919u + 13) % n_cand)];
    std::copy(scr.begin(), scr.end(), cand.begin());
    uint32_t round = 0;
    for (unsigned long long unresolved = n_cand; unresolved; ++round) {
        unsigned long long left = 0;
        LAUNCH((n_cand + 3) / 4, 4, k_diamond_mark(e.data(), n, round, cand.data(), cstate.data(), n_cand, nrank.data(), indeg.data(), inmin.data(), inmax.data(), mark.data()));
        for (uint32_t k = 0; k < n_cand; ++k) {
            if (cstate[k] != TS_UNRESOLVED) continue;
            const DiamondFoot d = diamond_foot(e.data(), n, indeg.data(), inmin.data(), inmax.data(), cand[k]);
            for (int i = 0; i < 4; ++i) if (!d.ok || mark[d.f[i]] == ~0ull) { printf("unwritten\n"); return 0; }
        }
        LAUNCH((n_cand + 3) / 4, 4, k_diamond_resolve(e.data(), n, round, cand.data(), cstate.data(), n_cand, nrank.data(), outdeg.data(), indeg.data(), inmin.data(), inmax.data(), mark.data(), eflag.data(), removed.data(), &left, cnt));
        if (left >= unresolved) { printf("stuck\n"); return 0; }
        unresolved = left;
    }
    LAUNCH(3, 4, k_diamond_nodes(n, n_nodes, eflag.data(), keep.data(), nrank.data(), removed.data(), nrank_out.data(), cnt));
    for (uint32_t i = 0; i < n; ++i) putchar('0' + eflag[i]);
    for (uint32_t i = 0; i < n; ++i) if (keep[i] != (eflag[i] == 0)) { printf("\nkeep\n"); return 0; }
    printf("\n%llu %llu %llu %llu %llu %llu %u\n", cnt[DC_INVALID], cnt[DC_CAND], cnt[DC_DIAMONDS], cnt[DC_NODES], cnt[DC_REMOVED], cnt[DC_KEPT], round);
    std::vector<std::pair<unsigned long long, uint32_t>> left;
    for (uint32_t i = 0; i < n_nodes; ++i) if (nrank_out[i] != NODE_NO_RANK) left.emplace_back(nrank_out[i], i);
    std::sort(left.begin(), left.end());
    for (auto& p : left) printf("%u ", p.second);
    printf("\n");
    return 0;
}
