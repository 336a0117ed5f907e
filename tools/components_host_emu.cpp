// Host emulation of phasm_amd/csrc/components.hip.h for tests/test_components_host_emulation.py: the kernels compiled as
// plain C++ with ONE lane per wave (threads run one after another), so a machine without a GPU checks their indexing and
// logic -- the sort of the rank words, the ranks of the edge ends, the hook and jump rounds, the numbering of the roots,
// the labels and the table -- against the goldens, under the host sanitizers.  The launches follow run_components
// (c_api.hip): the same memsets, and the round cap, the batches and the stop at the first round that lowers no word come
// from the functions of components.hip.h that run_components itself launches by.  The workspaces start as a call before
// could have left them.  Every loop here and in the kernels is bounded by a count.
//   stdin:  n_total n_edges n_order, one "u v" line per edge, the nodes in node order (node ids < n_total; ids at or
//           above the reads are merged nodes: the kernels do not tell them apart)
//   stdout: "invalid N" alone, or: the counters order, components, singletons, max nodes, max edges, rounds, batches, cap;
//           the component of every rank; the component of every edge; per component "first_node n_nodes n_edges;"
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include <algorithm>
#define __global__
#define __device__
#define __shared__ static
#define __restrict__
#define __launch_bounds__(x)
struct D3 { uint32_t x; };
static D3 threadIdx, blockIdx, blockDim, gridDim;
static inline void __syncthreads() {}
template <class T, class V> T atomicAdd(T* p, V v) { T o = *p; *p = (T)(*p + (T)v); return o; }
template <class T> T atomicMin(T* p, T v) { T o = *p; if (v < o) *p = v; return o; }
template <class T> T atomicMax(T* p, T v) { T o = *p; if (v > o) *p = v; return o; }
template <class T> T __shfl_xor(T v, int, int) { return v; }
namespace po {
constexpr int WAVE = 1;
struct Edge { uint32_t u, v; int32_t weight, overlap_len; };
constexpr unsigned long long NODE_NO_RANK = ~0ull;
static inline uint32_t lane_id() { return 0; }
static inline uint64_t wave_sum64(uint64_t v) { return v; }
template <int N> void block_add(const uint64_t (&v)[N], unsigned long long* c) { for (int k = 0; k < N; ++k) c[k] += v[k]; }
}
#include "../phasm_amd/csrc/merge.hip.h"
#include "../phasm_amd/csrc/components.hip.h"
using namespace po;
#define LAUNCH(grid, block, ...) do { gridDim.x = (grid); blockDim.x = (block); for (uint32_t b_ = 0; b_ < (grid); ++b_) for (uint32_t t_ = 0; t_ < (block); ++t_) { blockIdx.x = b_; threadIdx.x = t_; __VA_ARGS__; } } while (0)
int main() {
    uint32_t n_total, n, n_order_in;
    if (scanf("%u %u %u", &n_total, &n, &n_order_in) != 3) return 1;
    std::vector<Edge> e(n + 1);
    for (uint32_t i = 0; i < n; ++i) { if (scanf("%u %u", &e[i].u, &e[i].v) != 2) return 1; e[i].weight = 100; e[i].overlap_len = 17; }
    std::vector<unsigned long long> nrank(n_total + 1, NODE_NO_RANK);
    for (uint32_t i = 0; i < n_order_in; ++i) { uint32_t x; if (scanf("%u", &x) != 1 || x >= n_total) return 1; nrank[x] = ((unsigned long long)(3u * i + 5) << 2) | (i & 3); }
    const uint32_t pad = merge_sort_pad(n_total);
    const uint32_t nn = n_total + 2;
    std::vector<unsigned long long> key(pad, 7);
    std::vector<uint32_t> val(pad, 0xDEADu), rank_of(nn, 0xFFFFFFFFu), p(nn, 0xDEADu), index(nn, 0xDEADu), comp(nn, 0xDEADu), ecomp(n + 1, 0xDEADu);
    std::vector<uint8_t> root(nn, 9);
    std::vector<EdgeRanks> ends(n + 1, EdgeRanks{0xDEADu, 0xDEADu});
    std::vector<Component> table(nn, Component{0xDEADu, 0xDEADu, 0xDEADull});
    unsigned long long cnt[16] = {};
    LAUNCH((pad + 3) / 4, 4, k_cc_keys(nrank.data(), n_total, pad, key.data(), val.data()));
    merge_sort_steps(n_total, [&](uint32_t j, uint32_t k) { LAUNCH((pad + 3) / 4, 4, k_merge_bitonic(key.data(), val.data(), pad, j, k)); });
    LAUNCH((pad + 3) / 4, 4, k_cc_init(key.data(), val.data(), pad, n_total, p.data(), rank_of.data(), cnt));
    if (n) LAUNCH(3, 4, k_cc_ends(e.data(), n, n_total, rank_of.data(), ends.data(), cnt));
    if (cnt[KC_INVALID]) { printf("invalid %llu\n", cnt[KC_INVALID]); return 0; }
    if (cnt[KC_ORDER] != n_order_in) { printf("order\n"); return 0; }
    const uint32_t n_order = (uint32_t)cnt[KC_ORDER];
    const uint64_t cap = cc_round_cap(n_order);
    uint64_t launched = 0;
    uint32_t rounds = 0, batches = 0;
    bool done = n_order == 0;
    while (!done && launched < cap) {
        const uint32_t batch = (uint32_t)std::min<uint64_t>(CC_BATCH, cap - launched);
        unsigned long long rcnt[CC_BATCH] = {};
        for (uint32_t j = 0; j < batch; ++j, ++launched) {
            if (n) LAUNCH(3, 4, k_cc_hook(ends.data(), n, n_order, p.data(), rcnt + j));
            LAUNCH(3, 4, k_cc_jump(n_order, p.data(), rcnt + j));
        }
        uint64_t words[CC_BATCH];
        for (uint32_t j = 0; j < CC_BATCH; ++j) words[j] = rcnt[j];
        ++batches;
        done = cc_rounds_done(words, batch, rounds);
    }
    if (!done) { printf("cap\n"); return 0; }
    if (n_order) LAUNCH(3, 4, k_cc_roots(p.data(), n_order, root.data()));
    uint32_t n_comp = 0;
    for (uint32_t r = 0; r < n_order; ++r) { index[r] = n_comp; n_comp += root[r]; }   // (prefix_sum of the library)
    if (n_comp) {
        std::memset(table.data(), 0, (size_t)n_comp * sizeof(Component));
        LAUNCH(3, 4, k_cc_label_nodes(p.data(), index.data(), val.data(), n_order, n_comp, comp.data(), table.data()));
        if (n) LAUNCH(3, 4, k_cc_label_edges(ends.data(), n, n_order, n_comp, comp.data(), ecomp.data(), table.data()));
        LAUNCH(3, 4, k_cc_max(table.data(), n_comp, cnt));
    }
    printf("%u %u %llu %llu %llu %u %u %llu\n", n_order, n_comp, cnt[KC_SINGLE], cnt[KC_MAXN], cnt[KC_MAXE], rounds, batches,
           (unsigned long long)cap);
    for (uint32_t r = 0; r < n_order; ++r) printf("%u ", comp[r]);
    printf("\n");
    for (uint32_t i = 0; i < n; ++i) printf("%u ", ecomp[i]);
    printf("\n");
    for (uint32_t c = 0; c < n_comp; ++c) printf("%u %u %llu;", table[c].first_node, table[c].n_nodes, table[c].n_edges);
    printf("\n");
    return 0;
}
