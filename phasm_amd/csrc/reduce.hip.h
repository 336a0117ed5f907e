// Device side of the first two operations of `phasm layout` stage 2:
//   remove_transitive_edges (Myers' reduction)   phasm/assembly_graph.py:182-264
//   g.remove_edges_from(edges_to_remove)         phasm/cli/assembler.py:158
//   make_symmetric                               phasm/assembly_graph.py:429-443
// on the edge array po_layout_edges left in HBM.
//
// The reference walks the nodes in graph order with one shared node_state map.  Its decision for node v reads the
// state of v's neighbours only, and sets every one of them to IN_PLAY first (assembly_graph.py:228-229), so the
// result is a function of adj[v] and adj[w] for w in adj[v]: one independent task per node.  What does matter is the
// ORDER of every adjacency list -- sort_adjacency_lists (assembly_graph.py:48-55) sorts by weight, stably over the
// OrderedDict's insertion order -- because the walk over w skips a w that an earlier w eliminated (:231-232) and
// "first" means position 0 of adj[w] (:244-256).  So the lists are built in ascending (weight, rank) order, rank =
// the first input row that wrote the edge (add_edge on an existing edge keeps its place).
//   k_reduce_degree / _scatter / _order   CSR by source node, ordered by (weight, rank); a second index per node
//                                         ordered by target id serves the membership look-ups
//   k_reduce_mark                         one wave per node v: the three loops of assembly_graph.py:228-262
//   k_reduce_symmetric                    flag byte per edge: 0 kept, 1 transitive, 2 twin (v^1, u^1) gone
//   k_reduce_emit                         the kept edges, in stage-1 order
#pragma once

namespace po {

constexpr int RED_LDS_DEG = 1024;  // out-degree up to which a node's target ids and states sit in LDS (5 KB per wave)
enum { RC_TRANSITIVE = 0, RC_ASYMMETRIC = 1, RC_MAXDEG = 2, RC_INVALID = 3, RC_N = 4 };
// NodeState, assembly_graph.py:20-23 (VACANT never shows: every neighbour of v is set IN_PLAY first)
enum : uint8_t { NS_IN_PLAY = 1, NS_ELIMINATED = 2 };

// out-degree histogram
__global__ __launch_bounds__(256) void k_reduce_degree(const Edge* __restrict__ edges, uint32_t n_edges, uint32_t n_nodes,
                                                       uint32_t* __restrict__ deg, unsigned long long* __restrict__ counters) {
    uint64_t c[1] = {0};
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        const uint32_t u = edges[e].u, v = edges[e].v;
        if (u >= n_nodes || v >= n_nodes) {
            c[0] += 1;
            continue;
        }
        atomicAdd(&deg[u], 1u);
    }
    const uint64_t s = wave_sum64(c[0]);
    if (lane_id() == 0 && s) atomicAdd(&counters[RC_INVALID], (unsigned long long)s);
}

__global__ __launch_bounds__(256) void k_reduce_maxdeg(const uint32_t* __restrict__ deg, uint32_t n_nodes,
                                                       unsigned long long* __restrict__ counters) {
    uint32_t m = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_nodes; i += gridDim.x * blockDim.x) m = max(m, deg[i]);
    for (int d = WAVE / 2; d; d >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d));
    if (lane_id() == 0 && m) atomicMax(&counters[RC_MAXDEG], (unsigned long long)m);
}

// Every edge takes some slot of its source node's range.  WHICH one depends on the order of the atomics and is
// forgotten again by k_reduce_order; the slot only brings a node's (key, target, edge) triples side by side.
__global__ __launch_bounds__(256) void k_reduce_scatter(const Edge* __restrict__ edges, const uint32_t* __restrict__ rank,
                                                        uint32_t n_edges, const uint32_t* __restrict__ off,
                                                        uint32_t* __restrict__ cursor, unsigned long long* __restrict__ tkey,
                                                        uint32_t* __restrict__ ttgt, uint32_t* __restrict__ teid) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_edges) return;
    const Edge ed = edges[e];
    const uint32_t s = off[ed.u] + atomicAdd(&cursor[ed.u], 1u);
    // signed weight -> unsigned order; rank = first writer row (table path) or the emission index (adjacent path)
    tkey[s] = ((unsigned long long)((uint32_t)ed.weight ^ 0x80000000u) << 32) | (rank ? rank[e] : e);
    ttgt[s] = ed.v;
    teid[s] = e;
}

// Final place of every edge in its node's two lists = the number of the node's edges that come before it: in
// (weight, rank) order for the walk, in target order for the look-ups.  Both keys are total (the edge index breaks
// what ties could be left), so the result is the same permutation whatever k_reduce_scatter's atomics did.  Any
// out-degree works; the threads of a node read the same slots, which the caches serve.
__global__ __launch_bounds__(256) void k_reduce_order(const Edge* __restrict__ edges, uint32_t n_edges,
                                                      const uint32_t* __restrict__ off, const uint32_t* __restrict__ deg,
                                                      const unsigned long long* __restrict__ tkey,
                                                      const uint32_t* __restrict__ ttgt, const uint32_t* __restrict__ teid,
                                                      uint32_t* __restrict__ ctgt, int32_t* __restrict__ cw,
                                                      uint32_t* __restrict__ ceid, uint32_t* __restrict__ cidpos,
                                                      uint32_t* __restrict__ stgt, uint32_t* __restrict__ seid) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_edges) return;
    const uint32_t e = teid[s];
    const Edge ed = edges[e];
    const unsigned long long key = tkey[s];
    const uint32_t base = off[ed.u], d = deg[ed.u];
    uint32_t pw = 0, pi = 0;
    for (uint32_t t = 0; t < d; ++t) {
        const unsigned long long k = tkey[base + t];
        const uint32_t x = ttgt[base + t], e2 = teid[base + t];
        pw += (k < key) | ((k == key) & (e2 < e));
        pi += (x < ed.v) | ((x == ed.v) & (e2 < e));
    }
    ctgt[base + pw] = ed.v;
    cw[base + pw] = ed.weight;
    ceid[base + pw] = e;
    cidpos[base + pw] = pi;
    stgt[base + pi] = ed.v;
    seid[base + pi] = e;
}

// index of x in the ascending ids[0..d), or -1
template <typename P>
__device__ inline int reduce_find(P ids, uint32_t d, uint32_t x) {
    uint32_t lo = 0, hi = d;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (ids[mid] < x) lo = mid + 1; else hi = mid;
    }
    return (lo < d && ids[lo] == x) ? (int)lo : -1;
}

// The three loops of remove_transitive_edges for node v (assembly_graph.py:228-262) by ONE wave (the block).
// ids = v's targets in ascending order, state = one NodeState byte per entry of ids: both in LDS, or -- a node with
// more than RED_LDS_DEG out-edges -- in global memory (ids = the CSR's own target-ordered list, state = the node's
// range of a workspace with one byte per edge).  States only ever go IN_PLAY -> ELIMINATED, so the lanes store bytes
// without atomics; the barrier between two w makes the stores of one w visible to the test of the next.
template <typename PI, typename PS>
__device__ inline void reduce_mark_node(uint32_t base, uint32_t d, PI ids, PS state, int32_t fuzz,
                                        const uint32_t* __restrict__ off, const uint32_t* __restrict__ deg,
                                        const uint32_t* __restrict__ ctgt, const int32_t* __restrict__ cw,
                                        const uint32_t* __restrict__ ceid, const uint32_t* __restrict__ cidpos,
                                        uint8_t* __restrict__ flag1) {
    const uint32_t lane = threadIdx.x;
    // longest_edge + length_fuzz, :225-226 (the last entry of the sorted list)
    const long long limit = (long long)cw[base + d - 1] + fuzz;
    // :231-240 -- sequential over w: a w that an earlier w eliminated is skipped
    for (uint32_t k = 0; k < d; ++k) {
        if (state[cidpos[base + k]] == NS_IN_PLAY) {   // (the same byte for every lane, read behind the barrier)
            const uint32_t w = ctgt[base + k];
            const long long wv = cw[base + k];
            const uint32_t wb = off[w], wd = deg[w];
            for (uint32_t j = lane; j < wd; j += WAVE) {
                // adj[w] ascends by weight: behind the first sum above the limit every sum is above it
                if (wv + (long long)cw[wb + j] > limit) break;
                const int i = reduce_find(ids, d, ctgt[wb + j]);
                if (i >= 0) state[i] = NS_ELIMINATED;
            }
        }
        __syncthreads();
    }
    // :242-256 -- every w, whatever its state: position 0 of adj[w], and every x with weight(w, x) < fuzz (a prefix
    // of the ascending list).  No order between the w: one lane per w.
    for (uint32_t k = lane; k < d; k += WAVE) {
        const uint32_t w = ctgt[base + k];
        const uint32_t wb = off[w], wd = deg[w];
        for (uint32_t j = 0; j < wd; ++j) {
            if (j > 0 && cw[wb + j] >= fuzz) break;
            const int i = reduce_find(ids, d, ctgt[wb + j]);
            if (i >= 0) state[i] = NS_ELIMINATED;
        }
    }
    __syncthreads();
    // :258-262
    for (uint32_t k = lane; k < d; k += WAVE) flag1[ceid[base + k]] = state[cidpos[base + k]] == NS_ELIMINATED;
}

__global__ __launch_bounds__(WAVE) void k_reduce_mark(uint32_t n_nodes, int32_t fuzz, const uint32_t* __restrict__ off,
                                                      const uint32_t* __restrict__ deg, const uint32_t* __restrict__ ctgt,
                                                      const int32_t* __restrict__ cw, const uint32_t* __restrict__ ceid,
                                                      const uint32_t* __restrict__ cidpos, const uint32_t* __restrict__ stgt,
                                                      uint8_t* __restrict__ gstate, uint8_t* __restrict__ flag1) {
    __shared__ uint32_t s_ids[RED_LDS_DEG];
    __shared__ uint8_t s_state[RED_LDS_DEG];
    const uint32_t v = blockIdx.x;
    if (v >= n_nodes) return;
    const uint32_t d = deg[v];
    if (d == 0) return;
    const uint32_t base = off[v];
    // :228-229 -- every neighbour IN_PLAY
    if (d <= (uint32_t)RED_LDS_DEG) {
        for (uint32_t i = threadIdx.x; i < d; i += WAVE) {
            s_ids[i] = stgt[base + i];
            s_state[i] = NS_IN_PLAY;
        }
        __syncthreads();
        reduce_mark_node<const uint32_t*, uint8_t*>(base, d, s_ids, s_state, fuzz, off, deg, ctgt, cw, ceid, cidpos, flag1);
    } else {
        for (uint32_t i = threadIdx.x; i < d; i += WAVE) gstate[base + i] = NS_IN_PLAY;
        __syncthreads();
        reduce_mark_node<const uint32_t*, uint8_t*>(base, d, stgt + base, gstate + base, fuzz, off, deg, ctgt, cw, ceid, cidpos,
                                                    flag1);
    }
}

// make_symmetric on the graph without its transitive edges (assembly_graph.py:439-441): (u, v) goes iff (v^1, u^1)
// is not an edge any more.  One pass over the edge set as it stands, no fixpoint.  Reads flag1 only, writes flags.
__global__ __launch_bounds__(256) void k_reduce_symmetric(const Edge* __restrict__ edges, uint32_t n_edges,
                                                          const uint32_t* __restrict__ off, const uint32_t* __restrict__ deg,
                                                          const uint32_t* __restrict__ stgt, const uint32_t* __restrict__ seid,
                                                          const uint8_t* __restrict__ flag1, uint8_t* __restrict__ flags,
                                                          uint8_t* __restrict__ keep, unsigned long long* __restrict__ counters) {
    uint64_t c[2] = {0, 0};
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        uint32_t f = flag1[e];
        if (!f) {
            const Edge ed = edges[e];
            const uint32_t a = ed.v ^ 1u;
            const uint32_t base = off[a];
            const int i = reduce_find(stgt + base, deg[a], ed.u ^ 1u);
            if (i < 0 || flag1[seid[base + i]]) f = 2;
        }
        flags[e] = (uint8_t)f;
        keep[e] = f == 0;
        c[0] += f == 1;
        c[1] += f == 2;
    }
    block_add<2>(c, counters);
}

__global__ __launch_bounds__(256) void k_reduce_emit(const Edge* __restrict__ edges, const uint32_t* __restrict__ rank,
                                                     uint32_t n_edges, const uint8_t* __restrict__ keep,
                                                     const uint32_t* __restrict__ koff, Edge* __restrict__ kept,
                                                     uint32_t* __restrict__ kept_rank) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_edges || !keep[e]) return;
    kept[koff[e]] = edges[e];
    if (kept_rank) kept_rank[koff[e]] = rank[e];
}

}  // namespace po
