// Host emulation of phasm_amd/csrc/tips.hip.h for tests/test_tips_host_emulation.py: the kernels compiled as plain C++
// with ONE lane per wave (threads run one after another), so a machine without a GPU checks their indexing and logic --
// degrees and id sums, the rounds of both tip passes, the hash table of the symmetry pass, the node pass -- against the
// goldens, under the host sanitizers.  The candidate list of every pass is scrambled before the rounds: the answer must
// not depend on its order.  Threads of k_tips_resolve run one after another, so a later thread sees the removals of an
// earlier one of the same round -- one of the interleavings the device may produce.
//   stdin:  n_nodes L B n_edges n_order, then one "u v weight" line per edge, then the nodes in node order
//   stdout: the flag digits; the counters in, out, asym, invalid, nodes, isolated; candidates and rounds of both passes;
//           the nodes left, in order
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
using namespace po;
int main() {
    uint32_t n_nodes, L, n, n_order; int B;
    if (scanf("%u %u %d %u %u", &n_nodes, &L, &B, &n, &n_order) != 5) return 1;
    std::vector<Edge> e(n);
    for (uint32_t i = 0; i < n; ++i) { if (scanf("%u %u %d", &e[i].u, &e[i].v, &e[i].weight) != 3) return 1; e[i].overlap_len = 0; }
    std::vector<unsigned long long> nrank(n_nodes, NODE_NO_RANK), nrank_out(n_nodes, 7), mark(n_nodes);
    for (uint32_t i = 0; i < n_order; ++i) { uint32_t x; if (scanf("%u", &x) != 1 || x >= n_nodes) return 1; nrank[x] = ((unsigned long long)(3u * i + 5) << 2) | (i & 3); }
    const uint32_t n_slots = 2 * n + 64;
    std::vector<uint32_t> outdeg(n_nodes, 0), outsum(n_nodes, 0), indeg(n_nodes, 0), insum(n_nodes, 0), cand(n_nodes + 1), tval(n_slots, 99);
    std::vector<unsigned long long> tkey(n_slots, EDGE_EMPTY);
    // (the workspaces start as a call before could have left them)
    std::vector<uint8_t> cstate(n_nodes + 1, 9), eflag(n + 1, 9), flags(n + 1, 9), keep(n + 1, 9), alive(n_nodes + 1, 0);
    unsigned long long cnt[16] = {};
    LAUNCH(3, 4, k_tips_degree(e.data(), n, n_nodes, outdeg.data(), outsum.data(), indeg.data(), insum.data(), eflag.data(), cnt));
    LAUNCH(3, 4, k_tips_insert(e.data(), n, tkey.data(), tval.data(), n_slots));
    if (cnt[TC_INVALID]) { printf("invalid\n"); return 0; }
    const uint32_t max_len = std::min(L, n_nodes);
    unsigned long long stats[4];
    for (int rev = 0; rev < 2; ++rev) {
        TipSide g = rev ? TipSide{indeg.data(), insum.data(), outdeg.data(), outsum.data()} : TipSide{outdeg.data(), outsum.data(), indeg.data(), insum.data()};
        std::fill(mark.begin(), mark.end(), ~0ull);
        cnt[TC_CAND] = 0;
        LAUNCH((n_nodes + 3) / 4, 4, k_tips_candidates(n_nodes, nrank.data(), g.fdeg, g.bdeg, cand.data(), cstate.data(), cnt));
        const uint32_t n_cand = (uint32_t)cnt[TC_CAND];
        std::vector<uint32_t> scr(n_cand);
        for (uint32_t t = 0; t < n_cand; ++t) scr[t] = cand[n_cand % 7919u == 0 ? t : (uint32_t)(((uint64_t)t * 7919u + 13) % n_cand)];
        std::copy(scr.begin(), scr.end(), cand.begin());
        uint32_t round = 0;
        for (unsigned long long unresolved = n_cand; unresolved; ++round) {
            unsigned long long left = 0;
            LAUNCH((n_cand + 3) / 4, 4, k_tips_mark(e.data(), n, rev, max_len, round, cand.data(), cstate.data(), n_cand, nrank.data(), g.fdeg, g.fsum, mark.data()));
            LAUNCH((n_cand + 3) / 4, 4, k_tips_resolve(e.data(), n, rev, max_len, B, round, (uint8_t)(rev + 1), cand.data(), cstate.data(), n_cand, nrank.data(), g, mark.data(), eflag.data(), &left));
            if (left >= unresolved) { printf("stuck\n"); return 0; }
            unresolved = left;
        }
        stats[2 * rev] = n_cand;
        stats[2 * rev + 1] = round;
    }
    LAUNCH(3, 4, k_tips_symmetric(e.data(), n, tkey.data(), tval.data(), n_slots, eflag.data(), flags.data(), keep.data(), cnt));
    LAUNCH(3, 4, k_tips_alive(e.data(), n, keep.data(), alive.data()));
    LAUNCH(3, 4, k_tips_nodes(n_nodes, nrank.data(), alive.data(), nrank_out.data(), cnt));
    for (uint32_t i = 0; i < n; ++i) putchar('0' + flags[i]);
    printf("\n%llu %llu %llu %llu %llu %llu\n%llu %llu %llu %llu\n", cnt[TC_IN], cnt[TC_OUT], cnt[TC_ASYM], cnt[TC_INVALID], cnt[TC_NODES],
           cnt[TC_ISOLATED], stats[0], stats[1], stats[2], stats[3]);
    std::vector<std::pair<unsigned long long, uint32_t>> left;
    for (uint32_t i = 0; i < n_nodes; ++i) if (nrank_out[i] != NODE_NO_RANK) left.emplace_back(nrank_out[i], i);
    std::sort(left.begin(), left.end());
    for (auto& p : left) printf("%u ", p.second);
    printf("\n");
    return 0;
}
