// Host emulation of phasm_amd/csrc/superbubbles.hip.h for tests/test_superbubbles_host_emulation.py: the kernels compiled as
// plain C++ with ONE lane per wave (threads run one after another), so a machine without a GPU checks their indexing and
// logic -- behind the ranks and the SCC stage (the kernels of components.hip.h and partition.hip.h, as run_superbubbles of
// c_api.hip launches them through scc_stage): the degrees and the lists of D, sources and sinks, the level rounds, the two
// trees level by level, the pairs, the enclosing bubbles, the discards, the labels, the sums and the table -- against the
// goldens, under the host sanitizers.  The launches follow run_superbubbles: the same memsets, the same bounds, the batches
// and the stop at the first round that changes nothing from round_phase of components.hip.h, which run_superbubbles itself
// launches by.  The workspaces start as a call before could have left them.  Every loop here and in the kernels is bounded
// by a count.  The stage itself lives in superbubble_stage_host_emu.h, which bubblechains_host_emu.cpp runs too.
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
#include "superbubble_stage_host_emu.h"

int main() {
    RankedInput g;
    std::vector<uint32_t> colour;
    const int status = ranked_input(g, colour);
    if (status >= 0) return status;
    const uint32_t n_order = g.n_order;
    SuperbubbleStage S;
    if (!S.run(g, colour)) return 0;
    if (!n_order) { printf("0 0 0 0 0 0 0 0 0 0 0\n0 0 0 0 0 0\n\n\n\n\n"); return 0; }
    printf("%u %u %llu %llu %llu %u %llu %llu %llu %llu %llu\n", n_order, S.n_scc, (unsigned long long)S.n_real,
           (unsigned long long)(S.n_real + (S.cnt[BC_R_EDGES] != 0) + (S.cnt[BC_RE_EDGES] != 0)),
           (unsigned long long)(S.n_dedges + S.cnt[BC_LOOPS] + S.cnt[BC_R_EDGES] + S.cnt[BC_RE_EDGES]), S.n_bubbles, S.cnt[BC_NESTED], S.cnt[BC_LOOPS],
           S.cnt[BC_DISCARDED], (unsigned long long)S.levels_f, (unsigned long long)S.levels_b);
    printf("%u %u %u %u %llu %llu\n", S.level_rounds, S.discard_rounds, S.ops.batches, S.ops.max_batch, (unsigned long long)S.beyond,
           (unsigned long long)S.per_level);
    for (uint32_t r = 0; r < n_order; ++r) printf("%u ", S.d_exit[r]);
    printf("\n");
    for (uint32_t r = 0; r < n_order; ++r) printf("%u ", S.d_inside[r]);
    printf("\n");
    for (uint32_t r = 0; r < n_order; ++r) printf("%u ", S.d_flags[r]);
    printf("\n");
    for (uint32_t i = 0; i < S.n_bubbles; ++i) printf("%u %u %u %u;", S.table[i].entrance, S.table[i].exit, S.table[i].n_inside, S.table[i].nested);
    printf("\n");
    return 0;
}
