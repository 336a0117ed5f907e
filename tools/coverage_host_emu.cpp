// Host emulation of phasm_amd/csrc/coverage.hip.h for tests/test_coverage_host_emulation.py: the kernels compiled as plain
// C++ with ONE lane per wave (threads run one after another), so a machine without a GPU checks their indexing and logic --
// node_of, the pair table and its bounded probes, the sums and counts, the fill of the lists, inclusion-exclusion per edge --
// against the goldens, under the host sanitizers.  The launches and the memsets follow run_coverage (c_api.hip); the table
// size comes from the function run_coverage itself sizes it by.
//   stdin:  n_ids n_paths n_members n_edges n_rows; n_ids lengths; n_paths offsets; n_paths merged lengths; the members;
//           one "u v weight" line per edge; one "a b" line per row
//   stdout: "invalid N" alone, or the counters nodes, pairs, largest set, zero paths; then one "sum path" line per edge
#include "host_emu.h"
namespace po {
struct Edge { uint32_t u, v; int32_t weight, overlap_len; };
struct Row { uint32_t a_idx, b_idx; int32_t astart, aend, bstart, bend; };
}
#include "../phasm_amd/csrc/coverage.hip.h"
using namespace po;
int main() {
    uint32_t n_ids, K, n_members, n, n_rows;
    if (scanf("%u %u %u %u %u", &n_ids, &K, &n_members, &n, &n_rows) != 5) return 1;
    std::vector<uint32_t> len(n_ids + 1, 0), moff(K + 2, 0xDEADu), member(n_members + 1, 0xDEADu);
    std::vector<long long> mlen(K + 1, -1);
    for (uint32_t i = 0; i < n_ids; ++i) if (scanf("%u", &len[i]) != 1) return 1;
    for (uint32_t k = 0; k < K; ++k) if (scanf("%u", &moff[k]) != 1) return 1;
    for (uint32_t k = 0; k < K; ++k) if (scanf("%lld", &mlen[k]) != 1) return 1;
    for (uint32_t i = 0; i < n_members; ++i) if (scanf("%u", &member[i]) != 1) return 1;
    std::vector<Edge> e(n + 1);
    for (uint32_t i = 0; i < n; ++i) { if (scanf("%u %u %d", &e[i].u, &e[i].v, &e[i].weight) != 3) return 1; e[i].overlap_len = 17; }
    std::vector<Row> rows(n_rows + 1);
    for (uint32_t i = 0; i < n_rows; ++i) { if (scanf("%u %u", &rows[i].a_idx, &rows[i].b_idx) != 2) return 1; rows[i].astart = rows[i].aend = rows[i].bstart = rows[i].bend = 0; }
    const uint32_t n_total = n_ids + K, nn = n_total + 1, n_slots = cov_table_slots(n_rows), n_list = 2 * n_rows + 1;
    const uint32_t nb = (n_total + 3) / 4;
    // (what run_coverage memsets starts clean; the other workspaces start as a call before could have left them)
    std::vector<uint32_t> used(nn, 0), node_of(nn, 0xFFFFFFFFu), setcnt(nn, 0), cur(nn, 0), off(nn, 0xDEADu), list(n_list, 0xDEADBEEFu);
    std::vector<unsigned long long> sum(nn, 0), table(n_slots, ~0ull);
    std::vector<EdgeCoverage> out(n + 1, EdgeCoverage{77, -77});
    unsigned long long cnt[16] = {};
    LAUNCH(3, 4, k_cov_mark(e.data(), n, n_total, used.data(), cnt));
    LAUNCH(nb, 4, k_cov_nodes(n_ids, n_total, used.data(), node_of.data(), cnt));
    if (n_members && K) LAUNCH((n_members + 3) / 4, 4, k_cov_members(member.data(), n_members, moff.data(), K, n_ids, used.data(), node_of.data(), cnt));
    if (n_rows) LAUNCH(3, 4, k_cov_insert(rows.data(), n_rows, n_ids, len.data(), node_of.data(), table.data(), n_slots, sum.data(), setcnt.data(), cnt));
    LAUNCH(2, 4, k_cov_max(setcnt.data(), n_total, cnt));
    if (cnt[CC_INVALID]) { printf("invalid %llu\n", cnt[CC_INVALID]); return 0; }
    uint64_t total = 0;
    for (uint32_t i = 0; i < n_total; ++i) { off[i] = (uint32_t)total; total += setcnt[i]; }   // (prefix_sum of the library)
    if (total != cnt[CC_PAIRS] || total >= n_list) { printf("sizes\n"); return 0; }
    const uint32_t n_pairs = (uint32_t)total;
    if (n_pairs) LAUNCH(3, 4, k_cov_fill(table.data(), n_slots, n_total, off.data(), cur.data(), list.data(), n_pairs));
    for (uint32_t i = 0; i < n_total; ++i) if (cur[i] != setcnt[i]) { printf("fill\n"); return 0; }
    LAUNCH(3, 4, k_cov_edges(e.data(), n, n_ids, n_total, len.data(), mlen.data(), table.data(), n_slots, sum.data(), setcnt.data(),
                             off.data(), list.data(), n_pairs, out.data(), cnt));
    printf("%llu %llu %llu %llu\n", cnt[CC_NODES], cnt[CC_PAIRS], cnt[CC_MAXSET], cnt[CC_ZERO]);
    for (uint32_t i = 0; i < n; ++i) printf("%llu %lld\n", out[i].read_length_sum, out[i].path_length);
    return 0;
}
