// Host emulation of phasm_amd/csrc/cyclic.hip.h for tests/test_cyclic_host_emulation.py: the kernels compiled as plain C++ with
// ONE lane per wave (threads run one after another), so a machine without a GPU checks their indexing and logic -- the flat
// graph of every level, the roots, the seeds of the discards, the merge, the cycle search, the outputs -- around the SCC stage
// and the superbubble stage of superbubble_stage_host_emu.h, which run on the flat graphs as they run on a graph, under the
// host sanitizers.  The launches follow run_superbubbles_all of c_api.hip: the same memsets, the same bounds, the same walk
// of the parents on the host.  The workspaces start as a call before could have left them.  Every loop is bounded by a count.
//   stdin:  n_total n_edges n_order, one "u v" line per edge, the nodes in node order
//   stdout: "invalid N" alone, "bound WHAT" alone, or: order, bubbles, nested, in non-singleton SCCs, split, split levels,
//           rootless, runs, certified, edge-filtered; batches, the largest batch, the most levels of a run, the most ranks of
//           a flat graph; the exit of every rank; the inside of every rank; the flags of every rank; per bubble
//           "entrance exit n_inside nested;"
#include "host_emu.h"
namespace po {
struct Edge { uint32_t u, v; int32_t weight, overlap_len; };
constexpr unsigned long long NODE_NO_RANK = ~0ull;
}
#include "../phasm_amd/csrc/merge.hip.h"
#include "../phasm_amd/csrc/components.hip.h"
#include "../phasm_amd/csrc/partition.hip.h"
#include "../phasm_amd/csrc/superbubbles.hip.h"
#include "../phasm_amd/csrc/cyclic.hip.h"
using namespace po;

#include "rank_host_emu.h"
#include "superbubble_stage_host_emu.h"

int main() {
    RankedInput g;
    std::vector<uint32_t> ident;
    const int status = ranked_input(g, ident);
    if (status >= 0) return status;
    const uint32_t n = g.n, n0 = g.n_order, nn = g.nn, n2 = 2 * g.nn;
    if (!n0) { printf("0 0 0 0 0 0 0 0 0 0\n0 0 0 0\n\n\n\n\n"); return 0; }
    unsigned long long cnt[16] = {};
    std::vector<uint32_t> sidx(nn, 0xDEADu), root_of(nn, 0xDEADu), scc0(nn, 0xDEADu), m_exit(nn, CC_NONE), m_inside(nn, CC_NONE),
        m_size(nn, CC_NONE), m_total(nn, CC_NONE), dist(nn, 0xDEADu), par(nn, 0xDEADu), din(nn, 0xDEADu), pin(nn, 0xDEADu),
        best_in(n2, 0xDEADu), best_out(n2, 0xDEADu), best_low(n2, 0xDEADu), d_exit(nn, 0xDEADu), d_inside(nn, 0xDEADu), roots(n0);
    std::vector<uint8_t> split(nn, 9), cyclic0(nn, 9), rootless(nn, 0), uncertain(nn, 9), is_root(nn, 9), filtered(nn, 9), loop(nn, 0),
        m_is_exit(nn, 0), m_filtered(nn, 0), m_root(nn, 9), d_flags(nn, 9);
    if (n) LAUNCH(3, 4, k_cy_loops(g.ends.data(), n, n0, loop.data()));
    for (uint32_t r = 0; r < n0; ++r) roots[r] = r;
    struct Rootless { uint32_t low; std::vector<uint32_t> cycle; bool done; };
    std::vector<Rootless> open_sccs;
    uint64_t n_split_max = 0, n_rootless = 0, n_certified = 0, most_flat = 0;
    uint32_t levels_max = 0, runs = 0, batches = 0, max_batch = 0;
    // a flat graph: the input's edges and counts, ranks and workspaces for twice the nodes
    RankedInput F;
    F.n_total = g.n_total; F.n = n; F.pad = g.pad; F.nn = n2;
    for (uint32_t run = 0;; ++run) {
        std::copy(roots.begin(), roots.end(), root_of.begin());
        for (auto* v : {&split, &uncertain, &filtered}) std::fill(v->begin(), v->begin() + n0, 0);
        uint32_t n_split = 0;
        SuperbubbleStage S;
        std::vector<uint32_t> orig;
        for (uint32_t level = 0;; ++level) {
            if (level > (uint64_t)n0 + 1) { printf("bound split levels\n"); return 0; }
            const uint32_t n_flat = n0 + n_split;
            uint64_t total = 0;
            for (uint32_t r = 0; r < n0; ++r) { sidx[r] = (uint32_t)total; total += split[r]; }   // the library's prefix_sum
            if (total != n_split) { printf("bound split ranks\n"); return 0; }
            F.ends.assign(n + 1, EdgeRanks{0xDEADu, 0xDEADu});
            F.val.assign(n2, 0xDEADu);
            orig.assign(n2, 0xDEADu);
            F.index.assign(n2, 0xDEADu);
            F.root.assign(n2, 9);
            if (n) LAUNCH(3, 4, k_cy_flat(g.ends.data(), n, n0, split.data(), sidx.data(), n_split, F.ends.data()));
            LAUNCH(3, 4, k_cy_ranks(n0, g.val.data(), split.data(), sidx.data(), n_split, F.val.data(), orig.data()));
            std::memset(F.cnt, 0, sizeof F.cnt);
            F.n_order = n_flat;
            most_flat = std::max<uint64_t>(most_flat, n_flat);
            S = SuperbubbleStage();
            std::vector<uint32_t> colour(n2, 0xDEADu);
            if (!S.scc_rounds(F, colour)) return 0;
            batches += S.ops.batches;   // (the SCC stage counts its batches in its own ops: none here, see SccEmu)
            if (level == 0) LAUNCH(3, 4, k_cy_level0(n0, S.n_scc, S.node_scc.data(), S.sccs.data(), S.scc.data(), scc0.data(), cyclic0.data()));
            if (level == 1) LAUNCH(3, 4, k_cy_uncertain(n0, S.n_scc, S.node_scc.data(), S.sccs.data(), scc0.data(), uncertain.data()));
            const uint64_t singles = F.cnt[PC_SINGLE];
            if (singles > S.n_scc || S.n_scc > n_flat) { printf("bound sccs\n"); return 0; }
            const uint32_t n_cyclic = S.n_scc - (uint32_t)singles;
            if (!n_cyclic) break;
            if (n_cyclic > n0 - n_split) { printf("bound roots\n"); return 0; }
            for (auto* v : {&best_in, &best_out, &best_low}) std::fill(v->begin(), v->begin() + S.n_scc, CC_NONE);
            LAUNCH(3, 4, k_cy_choose(n0, S.n_scc, S.node_scc.data(), S.sccs.data(), S.pflags.data(), best_in.data(), best_out.data(), best_low.data()));
            LAUNCH(3, 4, k_cy_apply(n0, S.n_scc, S.sccs.data(), best_in.data(), best_out.data(), best_low.data(),
                                    level == 0 ? root_of.data() : (const uint32_t*)nullptr, level == 0 && run == 0 ? rootless.data() : (uint8_t*)nullptr,
                                    split.data(), cnt));
            n_split += n_cyclic;
            levels_max = std::max(levels_max, level + 1);
        }
        n_split_max = std::max<uint64_t>(n_split_max, n_split);
        if (cnt[YC_BAD]) { printf("bound no root\n"); return 0; }
        if (run == 0) n_rootless = cnt[YC_ROOTLESS];
        const uint32_t n_flat = n0 + n_split;
        if (!S.dag(F, [&] {
                if (n) LAUNCH(3, 4, k_cy_seed_edges(g.ends.data(), n, n0, n_flat, S.exit_of.data(), orig.data(), filtered.data()));
                LAUNCH(3, 4, k_cy_seed_ranks(n0, n_flat, S.exit_of.data(), orig.data(), filtered.data(), S.dead.data(), m_filtered.data()));
                return true;
            }))
            return 0;
        batches += S.ops.batches;
        max_batch = std::max(max_batch, S.ops.max_batch);
        LAUNCH(3, 4, k_cy_merge(n0, n_flat, orig.data(), F.root.data(), S.exit_of.data(), S.inside.data(), S.total.data(), m_exit.data(),
                                m_inside.data(), m_size.data(), m_total.data(), m_is_exit.data()));
        ++runs;
        const bool more = n_rootless && (run == 0 || !open_sccs.empty());
        if (!more) break;
        if (run == 0) {
            uint64_t seen = 0;
            for (uint32_t r = 0; r < n0; ++r) {
                if (!rootless[r]) continue;
                ++seen;
                if (uncertain[r]) open_sccs.push_back(Rootless{r, {}, false});
                else ++n_certified;
            }
            if (seen != n_rootless) { printf("bound rootless\n"); return 0; }
            if (open_sccs.empty()) break;
            LAUNCH(3, 4, k_cy_bfs_init(n0, rootless.data(), uncertain.data(), is_root.data(), dist.data(), par.data(), din.data(), pin.data()));
            Batches ops;
            uint32_t rounds = 0;
            uint64_t ignored = 0;
            const int how = round_phase(ops, n0, [&](uint32_t j) {
                ops.note(j);
                if (n) LAUNCH(3, 4, k_cy_bfs_round(g.ends.data(), n, n0, is_root.data(), dist.data(), din.data(), ops.rcnt + j));
            }, rounds, ops.batches, ignored);
            if (how != ROUNDS_DONE) { printf("bound cycle search\n"); return 0; }
            batches += ops.batches;
            max_batch = std::max(max_batch, ops.max_batch);
            if (n) LAUNCH(3, 4, k_cy_bfs_parents(g.ends.data(), n, n0, is_root.data(), dist.data(), din.data(), par.data(), pin.data()));
            for (Rootless& x : open_sccs) {
                const uint32_t len = din[x.low];
                uint32_t v = pin[x.low];
                bool ok = len >= 1 && len <= n0;
                for (uint32_t i = 1; ok && i < len; ++i) {
                    ok = v < n0 && v != x.low;
                    if (ok) { x.cycle.push_back(v); v = par[v]; }
                }
                if (!ok || v != x.low) { printf("bound cycle walk\n"); return 0; }
                std::reverse(x.cycle.begin(), x.cycle.end());
            }
        } else {
            for (Rootless& x : open_sccs)
                if (!x.done && !uncertain[x.low]) { x.done = true; ++n_certified; }
        }
        bool any = false;
        for (Rootless& x : open_sccs) {
            if (x.done) continue;
            if (run >= x.cycle.size()) { x.done = true; continue; }
            roots[x.low] = x.cycle[run];
            any = true;
        }
        if (!any) break;
    }
    LAUNCH(3, 4, k_cy_final(n0, g.val.data(), m_exit.data(), m_inside.data(), m_is_exit.data(), loop.data(), m_filtered.data(), cyclic0.data(),
                            m_root.data(), d_exit.data(), d_inside.data(), d_flags.data(), cnt));
    uint32_t n_bubbles = 0;
    for (uint32_t r = 0; r < n0; ++r) { g.index[r] = n_bubbles; n_bubbles += m_root[r]; }
    std::vector<Bubble> table(nn, Bubble{0xDEADu, 0xDEADu, 0xDEADu, 0xDEADu});
    if (n_bubbles)
        LAUNCH(3, 4, k_sb_table(n0, n_bubbles, g.val.data(), m_root.data(), g.index.data(), m_exit.data(), m_inside.data(), m_total.data(),
                                table.data()));
    printf("%u %u %llu %llu %llu %u %llu %u %llu %llu\n", n0, n_bubbles, cnt[YC_NESTED], cnt[YC_CYCLIC], (unsigned long long)n_split_max, levels_max,
           (unsigned long long)n_rootless, runs, (unsigned long long)n_certified, cnt[YC_FILTERED]);
    printf("%u %u %u %llu\n", batches, max_batch, levels_max, (unsigned long long)most_flat);
    for (uint32_t r = 0; r < n0; ++r) printf("%u ", d_exit[r]);
    printf("\n");
    for (uint32_t r = 0; r < n0; ++r) printf("%u ", d_inside[r]);
    printf("\n");
    for (uint32_t r = 0; r < n0; ++r) printf("%u ", d_flags[r]);
    printf("\n");
    for (uint32_t i = 0; i < n_bubbles; ++i) printf("%u %u %u %u;", table[i].entrance, table[i].exit, table[i].n_inside, table[i].nested);
    printf("\n");
    return 0;
}
