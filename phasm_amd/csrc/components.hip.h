// Device side of the first step of `phasm chain`:
//   networkx.weakly_connected_component_subgraphs(g)          phasm/cli/assembler.py:289-304
// on a graph result (an edge result, a merged graph or a po_graph_from_edges result) in HBM.
//
// The scheme works on RANKS: the place of a node in the node order.  One parent word p[r] per rank, p[r] = r at the start.
//   k_cc_keys / k_merge_bitonic / k_cc_init   the rank words of the result, sorted: rank r -> node, node -> rank, p[r] = r
//   k_cc_ends                                 the two ranks of every edge; an end outside the node order is counted
//   k_cc_hook                                 per edge: pu = p[rank u], pv = p[rank v]; if they differ, atomicMin of the
//                                             lower into p[higher], p[rank u], p[rank v]
//   k_cc_jump                                 per rank: p[r] = min(p[r], p[p[r]])
//                                             Both count the words they lowered into the round's change word.  p[r] <= r
//                                             always, and p[r] is a rank of r's component; a round that lowers nothing has
//                                             p[u] == p[v] on every edge and p[p[r]] == p[r]: the root of a component is
//                                             its lowest rank.  No kernel loops along parents: the host bounds the rounds.
//   k_cc_roots                                root[r] = p[r] == r; an exclusive prefix sum numbers the components by
//                                             their lowest-ranked node
//   k_cc_label_nodes / _edges / k_cc_max      component per rank and per edge (that of u), the table (first node, nodes,
//                                             edges), singletons and the two maxima
// The parent words are READ with plain loads, which may see a word as it was earlier in the same launch (the L2 of another
// XCD holds the line): an older parent is a higher rank of the same component, so a round only does less with it, never
// wrong; the round that ends the loop wrote nothing, so it read every word as it is.  They are WRITTEN by atomicMin only.
// Integer atomics only: every output is the same on every run (the number of rounds is not an output of the partition).
#pragma once

namespace po {

enum { KC_INVALID = 0, KC_ORDER = 1, KC_SINGLE = 2, KC_MAXN = 3, KC_MAXE = 4, KC_N = 5 };
constexpr uint32_t CC_NONE = 0xFFFFFFFFu;
constexpr uint32_t CC_BATCH = 8;   // rounds per readback

struct Component {
    uint32_t first_node, n_nodes;
    unsigned long long n_edges;
};

struct EdgeRanks {
    uint32_t ru, rv;
};

// live + 2, `live` = the ranks a loop of rounds works on (all n_order of them here, the live ones of a phase of
// partition.hip.h): the words are final after at most `live` rounds, the round after that counts nothing
inline uint64_t cc_round_cap(uint64_t live) { return live + 2; }

// The words of one batch: word j = parent words lowered in round j.  Counts the rounds up to and including the first
// that lowered none; true when that round was met.
inline bool cc_rounds_done(const volatile uint64_t* words, uint32_t batch, uint32_t& rounds) {
    for (uint32_t j = 0; j < batch; ++j) {
        ++rounds;
        if (words[j] == 0) return true;
    }
    return false;
}

enum { ROUNDS_DONE = 0, ROUNDS_CAP = 1, ROUNDS_FAILED = 3 };   // (the values scc_drive of partition.hip.h hands on)

// One loop of rounds: in batches of CC_BATCH, one change word per round and one readback per batch, up to and including
// the first round whose word is 0 (the later rounds of its batch change nothing either), at most cc_round_cap(live) of
// them.  ops.begin(batch) clears the words, round(j) launches the round that counts into word j, ops.end(batch, words)
// brings the words to the host; `total` sums them.  The loop of po_layout_components, every phase of po_layout_partition,
// and what the host emulations of both launch by.
template <class Ops, class Round>
inline int round_phase(Ops& ops, uint64_t live, Round&& round, uint32_t& rounds, uint32_t& batches, uint64_t& total) {
    const uint64_t cap = cc_round_cap(live);
    uint64_t launched = 0;
    bool done = false;
    while (!done && launched < cap) {
        const uint32_t batch = (uint32_t)(cap - launched < CC_BATCH ? cap - launched : CC_BATCH);
        if (!ops.begin(batch)) return ROUNDS_FAILED;
        for (uint32_t j = 0; j < batch; ++j, ++launched) round(j);
        const volatile uint64_t* words = nullptr;
        if (!ops.end(batch, words)) return ROUNDS_FAILED;
        ++batches;
        for (uint32_t j = 0; j < batch; ++j) total += words[j];
        done = cc_rounds_done(words, batch, rounds);
    }
    return done ? ROUNDS_DONE : ROUNDS_CAP;
}

// the sort's input: the rank word of every node (reads, then merged nodes), all ones behind them
__global__ __launch_bounds__(256) void k_cc_keys(const unsigned long long* __restrict__ nrank, uint32_t n_total, uint32_t n_pad,
                                                 unsigned long long* __restrict__ key, uint32_t* __restrict__ val) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pad) return;
    key[i] = i < n_total ? nrank[i] : NODE_NO_RANK;
    val[i] = i;
}

// after the sort: place r holds the node of rank r (the ranked nodes come first)
__global__ __launch_bounds__(256) void k_cc_init(const unsigned long long* __restrict__ key, const uint32_t* __restrict__ val,
                                                 uint32_t n_pad, uint32_t n_total, uint32_t* __restrict__ p,
                                                 uint32_t* __restrict__ rank_of, unsigned long long* __restrict__ counters) {
    uint64_t c[1] = {0};
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_pad && key[r] != NODE_NO_RANK && val[r] < n_total) {
        p[r] = r;
        rank_of[val[r]] = r;
        c[0] = 1;
    }
    block_add<1>(c, counters + KC_ORDER);
}

__global__ __launch_bounds__(256) void k_cc_ends(const Edge* __restrict__ edges, uint32_t n_edges, uint32_t n_total,
                                                 const uint32_t* __restrict__ rank_of, EdgeRanks* __restrict__ er,
                                                 unsigned long long* __restrict__ counters) {
    uint64_t c[1] = {0};
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        const uint32_t u = edges[e].u, v = edges[e].v;
        const uint32_t ru = u < n_total ? rank_of[u] : CC_NONE, rv = v < n_total ? rank_of[v] : CC_NONE;
        const bool ok = ru != CC_NONE && rv != CC_NONE;
        er[e] = ok ? EdgeRanks{ru, rv} : EdgeRanks{CC_NONE, CC_NONE};
        c[0] += !ok;
    }
    const uint64_t s = wave_sum64(c[0]);
    if (lane_id() == 0 && s) atomicAdd(&counters[KC_INVALID], (unsigned long long)s);
}

__global__ __launch_bounds__(256) void k_cc_hook(const EdgeRanks* __restrict__ er, uint32_t n_edges, uint32_t n_order,
                                                 uint32_t* __restrict__ p, unsigned long long* __restrict__ changed) {
    uint64_t c[1] = {0};
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        const EdgeRanks x = er[e];
        if (x.ru >= n_order || x.rv >= n_order || x.ru == x.rv) continue;   // (a self-loop joins nothing)
        const uint32_t pu = p[x.ru], pv = p[x.rv];
        if (pu == pv) continue;
        const uint32_t lo = pu < pv ? pu : pv, hi = pu < pv ? pv : pu;
        if (hi >= n_order) continue;   // (never index on trust)
        c[0] += atomicMin(&p[hi], lo) > lo;
        c[0] += atomicMin(&p[x.ru], lo) > lo;
        c[0] += atomicMin(&p[x.rv], lo) > lo;
    }
    const uint64_t s = wave_sum64(c[0]);
    if (lane_id() == 0 && s) atomicAdd(changed, (unsigned long long)s);
}

__global__ __launch_bounds__(256) void k_cc_jump(uint32_t n_order, uint32_t* __restrict__ p, unsigned long long* __restrict__ changed) {
    uint64_t c[1] = {0};
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        const uint32_t q = p[r];
        if (q >= n_order) continue;
        const uint32_t g = p[q];
        if (g < q) c[0] += atomicMin(&p[r], g) > g;
    }
    const uint64_t s = wave_sum64(c[0]);
    if (lane_id() == 0 && s) atomicAdd(changed, (unsigned long long)s);
}

__global__ __launch_bounds__(256) void k_cc_roots(const uint32_t* __restrict__ p, uint32_t n_order, uint8_t* __restrict__ root) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) root[r] = p[r] == r;
}

__global__ __launch_bounds__(256) void k_cc_label_nodes(const uint32_t* __restrict__ p, const uint32_t* __restrict__ index,
                                                        const uint32_t* __restrict__ node_at, uint32_t n_order, uint32_t n_comp,
                                                        uint32_t* __restrict__ comp, Component* __restrict__ table) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        const uint32_t q = p[r];
        const uint32_t c = q < n_order ? index[q] : CC_NONE;
        if (c >= n_comp) {   // (cannot happen after a round that lowered nothing)
            comp[r] = CC_NONE;
            continue;
        }
        comp[r] = c;
        atomicAdd(&table[c].n_nodes, 1u);
        if (q == r) table[c].first_node = node_at[r];
    }
}

__global__ __launch_bounds__(256) void k_cc_label_edges(const EdgeRanks* __restrict__ er, uint32_t n_edges, uint32_t n_order,
                                                        uint32_t n_comp, const uint32_t* __restrict__ comp,
                                                        uint32_t* __restrict__ edge_comp, Component* __restrict__ table) {
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        const uint32_t ru = er[e].ru;
        const uint32_t c = ru < n_order ? comp[ru] : CC_NONE;
        edge_comp[e] = c;
        if (c < n_comp) atomicAdd(&table[c].n_edges, 1ull);
    }
}

__global__ __launch_bounds__(256) void k_cc_max(const Component* __restrict__ table, uint32_t n_comp,
                                                unsigned long long* __restrict__ counters) {
    uint64_t single = 0;
    unsigned long long mn = 0, me = 0;
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < n_comp; c += gridDim.x * blockDim.x) {
        const Component x = table[c];
        single += x.n_nodes == 1;
        mn = x.n_nodes > mn ? x.n_nodes : mn;
        me = x.n_edges > me ? x.n_edges : me;
    }
    const uint64_t s = wave_sum64(single);
    if (lane_id() == 0 && s) atomicAdd(&counters[KC_SINGLE], (unsigned long long)s);
    if (mn) atomicMax(&counters[KC_MAXN], mn);
    if (me) atomicMax(&counters[KC_MAXE], me);
}

}  // namespace po
