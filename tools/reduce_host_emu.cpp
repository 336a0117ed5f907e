// Host emulation of phasm_amd/csrc/reduce.hip.h for tests/test_reduce_host_emulation.py: the kernels compiled as plain
// C++ with ONE lane per wave (threads run one after another, barriers are no-ops), so a machine without a GPU checks
// their indexing and logic -- CSR order, both state placements of k_reduce_mark, the symmetry look-up -- against the
// goldens, under the host sanitizers.  What it cannot see: anything that needs lanes to run side by side.
//   stdin:  n_nodes fuzz n_edges, then one "u v weight rank" line per edge;  stdout: the flag digits, then the counters
#include "host_emu.h"
namespace po {
struct Edge { uint32_t u, v; int32_t weight, overlap_len; };
}
#include "../phasm_amd/csrc/reduce.hip.h"
using namespace po;
int main(int argc, char** argv) {
    // input: n_nodes fuzz n ; then n lines u v w rank ; output flags
    uint32_t n_nodes, n; int fuzz;
    if (scanf("%u %d %u", &n_nodes, &fuzz, &n) != 3) return 1;
    std::vector<Edge> e(n); std::vector<uint32_t> rank(n);
    for (uint32_t i = 0; i < n; ++i) { if (scanf("%u %u %d %u", &e[i].u, &e[i].v, &e[i].weight, &rank[i]) != 4) return 1; e[i].overlap_len = 0; }
    std::vector<uint32_t> deg(n_nodes + 1, 0), off(n_nodes + 1, 0), cur(n_nodes + 1, 0), ttgt(n), teid(n), ctgt(n), ceid(n), cidpos(n), stgt(n), seid(n), koff(n + 1);
    std::vector<int32_t> cw(n); std::vector<unsigned long long> tkey(n); unsigned long long cnt[16] = {};
    // (the workspace starts as a call before could have left it: a state that is not set again reads ELIMINATED)
    std::vector<uint8_t> gstate(n, NS_ELIMINATED), flag1(n, 99), flags(n, 99), keep(n);
    LAUNCH(3, 4, k_reduce_degree(e.data(), n, n_nodes, deg.data(), cnt));
    LAUNCH(2, 4, k_reduce_maxdeg(deg.data(), n_nodes, cnt));
    for (uint32_t i = 0, s = 0; i < n_nodes; ++i) { off[i] = s; s += deg[i]; }
    // scatter in a scrambled order: the result must not depend on it
    { gridDim.x = 1; blockDim.x = n; blockIdx.x = 0; for (uint32_t t = 0; t < n; ++t) { threadIdx.x = (uint32_t)(((uint64_t)t * 7919u + 13) % n); if (n % 7919u == 0) threadIdx.x = t; k_reduce_scatter(e.data(), rank.data(), n, off.data(), cur.data(), tkey.data(), ttgt.data(), teid.data()); } }
    LAUNCH((n + 3) / 4, 4, k_reduce_order(e.data(), n, off.data(), deg.data(), tkey.data(), ttgt.data(), teid.data(), ctgt.data(), cw.data(), ceid.data(), cidpos.data(), stgt.data(), seid.data()));
    LAUNCH(n_nodes, 1, k_reduce_mark(n_nodes, fuzz, off.data(), deg.data(), ctgt.data(), cw.data(), ceid.data(), cidpos.data(), stgt.data(), gstate.data(), flag1.data()));
    LAUNCH(3, 4, k_reduce_symmetric(e.data(), n, off.data(), deg.data(), stgt.data(), seid.data(), flag1.data(), flags.data(), keep.data(), cnt));
    for (uint32_t i = 0; i < n; ++i) putchar('0' + flags[i]);
    printf("\n%llu %llu %llu %llu\n", cnt[0], cnt[1], cnt[2], cnt[3]);
    return 0;
}
