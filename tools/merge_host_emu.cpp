// Host emulation of phasm_amd/csrc/merge.hip.h for tests/test_merge_host_emulation.py: the kernels compiled as plain C++
// with ONE lane per wave (threads run one after another), so a machine without a GPU checks their indexing and logic --
// degrees and links, the pointer-jumping rounds, the sort of the heads, the tables, the renamed edges, the ranks of the
// result -- against the goldens, under the host sanitizers.  The launches follow run_merge (c_api.hip): the same memsets,
// and the round cap, the batches, the stop at the first round that brings no node to a root and the steps of the sort
// come from the functions of merge.hip.h that run_merge itself launches by.  The list of heads is
// scrambled before the sort, and the workspaces start as a call before could have left them.  Every loop here and in
// the kernels is bounded by a count, so a graph of link cycles ends like any other.
//   stdin:  n_nodes n_edges n_order, one "u v weight overlap_len" line per edge, the nodes in node order, n_nodes lengths
//   stdout: the flag digits (or "invalid" / "overflow N" alone); the counters invalid, nodes, heads, merged, cycle,
//           longest, self-loops, overflow, kept and the rounds; the nodes of the result in order; offsets; members;
//           prefixes; lengths; the kept edges as "u v w o;"
#include "host_emu.h"
namespace po {
struct Edge { uint32_t u, v; int32_t weight, overlap_len; };
constexpr unsigned long long NODE_NO_RANK = ~0ull;
}
#include "../phasm_amd/csrc/merge.hip.h"
using namespace po;
int main() {
    uint32_t n_nodes, n, n_order;
    if (scanf("%u %u %u", &n_nodes, &n, &n_order) != 3) return 1;
    std::vector<Edge> e(n + 1), renamed(n + 1);
    for (uint32_t i = 0; i < n; ++i) if (scanf("%u %u %d %d", &e[i].u, &e[i].v, &e[i].weight, &e[i].overlap_len) != 4) return 1;
    std::vector<unsigned long long> nrank(n_nodes + 1, NODE_NO_RANK);
    for (uint32_t i = 0; i < n_order; ++i) { uint32_t x; if (scanf("%u", &x) != 1 || x >= n_nodes) return 1; nrank[x] = ((unsigned long long)(3u * i + 5) << 2) | (i & 3); }
    std::vector<uint32_t> len(n_nodes + 1, 0);
    for (uint32_t i = 0; i < n_nodes; ++i) if (scanf("%u", &len[i]) != 1) return 1;
    const uint32_t nn = n_nodes + 1, nb = (n_nodes + 3) / 4;
    std::vector<uint32_t> outdeg(nn, 0), indeg(nn, 0), oute(nn, 0xFFFFFFFFu), ine(nn, 0xFFFFFFFFu);
    // (the other workspaces start as a call before could have left them)
    std::vector<uint32_t> link(nn, 0xDEADu), back(nn, 0xDEADu), hlen(nn, 77), pathk(nn, 0xDEADu), npath(nn, 5), npos(nn, 5);
    std::vector<uint32_t> jb[2] = {std::vector<uint32_t>(nn, 0xDEADu), std::vector<uint32_t>(nn, 0xDEADu)};
    std::vector<uint32_t> hops[2] = {std::vector<uint32_t>(nn, 9), std::vector<uint32_t>(nn, 9)};
    std::vector<unsigned long long> ws[2] = {std::vector<unsigned long long>(nn, 9), std::vector<unsigned long long>(nn, 9)};
    std::vector<unsigned long long> hsum(nn, 9);
    const uint32_t max_heads = n_nodes / 2 + 1;
    uint32_t pad_cap = 1;
    while (pad_cap < max_heads) pad_cap <<= 1;
    std::vector<unsigned long long> hkey(pad_cap, ~0ull);
    std::vector<uint32_t> hval(pad_cap, 0xDEADu);
    std::vector<uint8_t> eflag(n + 1, 9), keep(n + 1, 9);
    unsigned long long cnt[16] = {};
    LAUNCH(3, 4, k_merge_degree(e.data(), n, n_nodes, outdeg.data(), indeg.data(), oute.data(), ine.data(), cnt));
    if (cnt[MC_INVALID]) { printf("invalid\n"); return 0; }
    LAUNCH(nb, 4, k_merge_links(e.data(), n, n_nodes, nrank.data(), outdeg.data(), indeg.data(), oute.data(), ine.data(), link.data(),
                                back.data(), jb[0].data(), hops[0].data(), ws[0].data(), hlen.data(), hkey.data(), hval.data(), cnt));
    const uint32_t K = (uint32_t)cnt[MC_HEADS];
    if (K > max_heads) { printf("heads\n"); return 0; }
    for (uint32_t t = 0; t + 1 < K; ++t) {   // any order of the compacted heads
        const uint32_t o = t + (uint32_t)(((uint64_t)t * 7919u + 13) % (K - t));
        std::swap(hkey[t], hkey[o]);
        std::swap(hval[t], hval[o]);
    }
    const uint32_t max_rounds = merge_round_cap(cnt[MC_NODES]);
    uint32_t launched = 0, rounds = 0;
    for (bool done = K == 0; !done && launched < max_rounds;) {
        const uint32_t batch = std::min<uint32_t>(MERGE_BATCH, max_rounds - launched);
        unsigned long long rcnt[MERGE_BATCH] = {};
        for (uint32_t j = 0; j < batch; ++j, ++launched) {
            const int a = merge_final_buffer(launched), b = a ^ 1;
            LAUNCH(nb, 4, k_merge_jump(n_nodes, back.data(), jb[a].data(), hops[a].data(), ws[a].data(), jb[b].data(), hops[b].data(),
                                       ws[b].data(), rcnt + j));
        }
        uint64_t words[MERGE_BATCH];
        for (uint32_t j = 0; j < MERGE_BATCH; ++j) words[j] = rcnt[j];
        done = merge_rounds_done(words, batch, rounds);
    }
    const int fin = merge_final_buffer(launched);
    const uint32_t pad = merge_sort_pad(K);
    LAUNCH(nb, 4, k_merge_tails(n_nodes, link.data(), back.data(), jb[fin].data(), hops[fin].data(), ws[fin].data(), hlen.data(),
                                hsum.data(), cnt));
    merge_sort_steps(K, [&](uint32_t j, uint32_t k) { LAUNCH((pad + 3) / 4, 4, k_merge_bitonic(hkey.data(), hval.data(), pad, j, k)); });
    std::vector<uint32_t> lens(K + 1, 9), moff(K + 2, 9);
    std::vector<long long> psum(K + 1, 9), mlen(K + 1, -1);
    LAUNCH((K + 3) / 4, 4, k_merge_number(K, n_nodes, hval.data(), hlen.data(), hsum.data(), pathk.data(), lens.data(), psum.data()));
    uint32_t n_members = 0;
    for (uint32_t k = 0; k < K; ++k) { moff[k] = n_members; n_members += lens[k]; }   // (prefix_sum of the library)
    if (n_members != cnt[MC_MERGED]) { printf("lengths\n"); return 0; }
    std::vector<uint32_t> member(n_members + 1, 0xDEADu);
    std::vector<int32_t> prefix(n_members + 1, -7);
    std::vector<unsigned long long> nrank_out(n_nodes + K + 1, 7);
    LAUNCH(nb, 4, k_merge_tables(e.data(), n, n_nodes, len.data(), link.data(), back.data(), jb[fin].data(), hops[fin].data(),
                                 ws[fin].data(), oute.data(), pathk.data(), moff.data(), K, n_members, member.data(), prefix.data(),
                                 mlen.data(), npath.data(), npos.data()));
    LAUNCH(3, 4, k_merge_ranks(n_nodes, K, nrank.data(), npath.data(), cnt, nrank_out.data()));
    LAUNCH(3, 4, k_merge_edges(e.data(), n, n_nodes, link.data(), npath.data(), psum.data(), renamed.data(), eflag.data(), keep.data(), cnt));
    if (cnt[MC_OVERFLOW]) { printf("overflow %llu\n", cnt[MC_OVERFLOW]); return 0; }
    for (uint32_t i = 0; i < n; ++i) putchar('0' + eflag[i]);
    for (uint32_t i = 0; i < n; ++i) if (keep[i] != (eflag[i] != 1)) { printf("\nkeep\n"); return 0; }
    printf("\n%llu %llu %llu %llu %llu %llu %llu %llu %llu %u\n", cnt[MC_INVALID], cnt[MC_NODES], cnt[MC_HEADS], cnt[MC_MERGED], cnt[MC_CYCLE],
           cnt[MC_MAXPATH], cnt[MC_SELF], cnt[MC_OVERFLOW], cnt[MC_KEPT], rounds);
    std::vector<std::pair<unsigned long long, uint32_t>> left;
    for (uint32_t i = 0; i < n_nodes + K; ++i) if (nrank_out[i] != NODE_NO_RANK) left.emplace_back(nrank_out[i], i);
    std::sort(left.begin(), left.end());
    for (auto& p : left) printf("%u ", p.second);
    printf("\n");
    for (uint32_t k = 0; k < K; ++k) printf("%u ", moff[k]);
    printf("%u\n", n_members);
    for (uint32_t i = 0; i < n_members; ++i) printf("%u ", member[i]);
    printf("\n");
    for (uint32_t i = 0; i < n_members; ++i) printf("%d ", prefix[i]);
    printf("\n");
    for (uint32_t k = 0; k < K; ++k) printf("%lld ", mlen[k]);
    printf("\n");
    for (uint32_t i = 0; i < n; ++i) if (keep[i]) printf("%u %u %d %d;", renamed[i].u, renamed[i].v, renamed[i].weight, renamed[i].overlap_len);
    printf("\n");
    // the (path, pos) of every member is its place in the tables
    for (uint32_t k = 0; k < K; ++k)
        for (uint32_t i = moff[k]; i < moff[k] + lens[k]; ++i)
            if (member[i] >= n_nodes || npath[member[i]] != k || npos[member[i]] != i - moff[k]) { printf("pos\n"); return 0; }
    return 0;
}
