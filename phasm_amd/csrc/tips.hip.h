// Device side of the tip removal of `phasm layout` stage 2:
//   remove_incoming_tips / remove_outgoing_tips   phasm/assembly_graph.py:267-394
//   make_symmetric                                phasm/assembly_graph.py:429-443
//   clean_graph                                   phasm/assembly_graph.py:446-453
// on an edge result (po_layout_edges, po_layout_reduce or po_layout_tips itself) in HBM.
//
// The reference visits the tips in the graph's node order, and every removal changes the degrees the next walk reads
// (assembly_graph.py:347-379), so the answer depends on that order.  The order is a rank per node (k_layout_node_rank,
// layout.hip.h); the walks run in ROUNDS that give the sequential answer:
//   a candidate = a node with no live in-edge and one live out-edge at the start of the pass (the only tips the
//   reference does not skip, :352); its CHAIN = the at most L + 2 nodes reached by following `out == 1` successors
//   whatever their in-degree; its WALK = the prefix of the chain the reference's loop (:358-372) visits on the graph as
//   it stands.  A removal lowers the in-degree of the walk's last node only; the other nodes of a removed path have
//   their single in-edge from the path itself, so no other chain runs through them and the out-degrees along a chain
//   never change within a pass.
//   k_tips_mark      every unresolved candidate writes its key (round, rank) into the mark word of every node of its
//                    chain, atomicMin; later rounds carry smaller keys, so the words need no reset in between
//   k_tips_resolve   a candidate whose walk holds its own key in every node is RESOLVED: no unresolved candidate of
//                    lower rank can ever touch a node it reads, and a resolved one of higher rank never read a node it
//                    writes.  It decides as the reference does and, if it is a tip, takes its edges out.
// The lowest unresolved candidate always resolves, so the rounds end.  The outgoing pass is the same code on the
// transposed degrees.  Degrees come with the SUM of the live edge ids per node and side: at degree 1 the sum is the
// edge, so a removal is two atomic subtractions per end.
//   k_tips_degree / _candidates   degrees, id sums, the candidate list of a pass (any order: the rank decides)
//   k_tips_insert / _symmetric    (u, v) -> edge id hash table; flag byte per edge: 0 kept, 1 incoming-tip edge,
//                                 2 outgoing-tip edge, 3 twin (v^1, u^1) gone
//   k_tips_alive / _nodes         nodes left without an edge are counted and lose their rank (clean_graph)
#pragma once

namespace po {

enum { TC_IN = 0, TC_OUT = 1, TC_ASYM = 2, TC_INVALID = 3, TC_NODES = 4, TC_ISOLATED = 5, TC_CAND = 6, TC_N = 7 };
constexpr unsigned long long NODE_NO_RANK = ~0ull;   // (row << 2 | slot) < 2^33 otherwise
constexpr int TIP_RANK_BITS = 33;
enum : uint8_t { TS_UNRESOLVED = 0, TS_RESOLVED = 1 };

// One side of the graph as a pass sees it: "forward" is the direction of the walk.
struct TipSide {
    uint32_t* fdeg;   // live edges leaving a node in walk direction
    uint32_t* fsum;   // sum of their ids
    uint32_t* bdeg;   // live edges entering a node in walk direction
    uint32_t* bsum;
};

__global__ __launch_bounds__(256) void k_tips_degree(const Edge* __restrict__ edges, uint32_t n_edges, uint32_t n_nodes,
                                                     uint32_t* __restrict__ outdeg, uint32_t* __restrict__ outsum,
                                                     uint32_t* __restrict__ indeg, uint32_t* __restrict__ insum,
                                                     uint8_t* __restrict__ eflag, unsigned long long* __restrict__ counters) {
    uint64_t c[1] = {0};
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        const uint32_t u = edges[e].u, v = edges[e].v;
        eflag[e] = 0;
        if (u >= n_nodes || v >= n_nodes) {
            c[0] += 1;
            continue;
        }
        atomicAdd(&outdeg[u], 1u);
        atomicAdd(&outsum[u], e);
        atomicAdd(&indeg[v], 1u);
        atomicAdd(&insum[v], e);
    }
    const uint64_t s = wave_sum64(c[0]);
    if (lane_id() == 0 && s) atomicAdd(&counters[TC_INVALID], (unsigned long long)s);
}

// tips = [n for n in g if in_degree(n) == 0] and the test out_degree(tip) == 1 (:347-353); a node without a rank is no
// node of the graph
__global__ __launch_bounds__(256) void k_tips_candidates(uint32_t n_nodes, const unsigned long long* __restrict__ nrank,
                                                         const uint32_t* __restrict__ fdeg, const uint32_t* __restrict__ bdeg,
                                                         uint32_t* __restrict__ cand, uint8_t* __restrict__ cstate,
                                                         unsigned long long* __restrict__ counters) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_nodes) return;
    if (nrank[n] == NODE_NO_RANK || bdeg[n] != 0 || fdeg[n] != 1) return;
    const uint32_t k = (uint32_t)atomicAdd(&counters[TC_CAND], 1ull);
    cand[k] = n;
    cstate[k] = TS_UNRESOLVED;
}

__device__ inline unsigned long long tip_key(uint32_t round, unsigned long long rank) {
    return ((unsigned long long)(0x7FFFFFFFu - round) << TIP_RANK_BITS) | rank;
}

// the node the one live forward edge of `curr` leads to (rev: the walk runs against the edges), and the edge
__device__ inline bool tip_step(const Edge* __restrict__ edges, uint32_t n_edges, const uint32_t* fsum, uint32_t curr, int rev,
                                uint32_t& e, uint32_t& next, int32_t& w) {
    e = fsum[curr];
    if (e >= n_edges) return false;   // (cannot happen while degree and sum agree; never index on trust)
    const Edge ed = edges[e];
    next = rev ? ed.u : ed.v;
    w = ed.weight;
    return true;
}

__global__ __launch_bounds__(256) void k_tips_mark(const Edge* __restrict__ edges, uint32_t n_edges, int rev, uint32_t max_len,
                                                   uint32_t round, const uint32_t* __restrict__ cand,
                                                   const uint8_t* __restrict__ cstate, uint32_t n_cand,
                                                   const unsigned long long* __restrict__ nrank, const uint32_t* fdeg,
                                                   const uint32_t* fsum, unsigned long long* __restrict__ mark) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_cand || cstate[k] != TS_UNRESOLVED) return;
    uint32_t curr = cand[k];
    const unsigned long long key = tip_key(round, nrank[curr]);
    atomicMin(&mark[curr], key);
    // the chain: max_len + 2 nodes at the most, the longest path the walk can build before the length bound ends it
    for (uint32_t len = 1; len < max_len + 2 && fdeg[curr] == 1; ++len) {
        uint32_t e, next;
        int32_t w;
        if (!tip_step(edges, n_edges, fsum, curr, rev, e, next, w)) break;
        curr = next;
        atomicMin(&mark[curr], key);
    }
}

// remove_incoming_tips for one tip, :355-379 (rev: remove_outgoing_tips, :296-321).  `which` = the flag of a removed
// edge.  The degrees of another candidate's nodes may change under this walk while that candidate takes its edges
// out; in-degrees only fall, so the walk then reaches further, never less far, and still meets the foreign mark that
// keeps this candidate unresolved.
__global__ __launch_bounds__(256) void k_tips_resolve(const Edge* __restrict__ edges, uint32_t n_edges, int rev, uint32_t max_len,
                                                      int32_t max_bases, uint32_t round, uint8_t which,
                                                      const uint32_t* __restrict__ cand, uint8_t* __restrict__ cstate,
                                                      uint32_t n_cand, const unsigned long long* __restrict__ nrank, TipSide g,
                                                      const unsigned long long* __restrict__ mark, uint8_t* __restrict__ eflag,
                                                      unsigned long long* __restrict__ unresolved) {
    uint64_t c[1] = {0};   // candidates left unresolved
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n_cand && cstate[k] == TS_UNRESOLVED) {
        const uint32_t s = cand[k];
        const unsigned long long key = tip_key(round, nrank[s]);
        uint32_t curr = s, len = 1;
        long long bases = 0;
        bool is_tip = true, mine = mark[s] == key;
        while (mine && g.fdeg[curr] == 1 && g.bdeg[curr] <= 1) {
            uint32_t e, next;
            int32_t w;
            if (!tip_step(edges, n_edges, g.fsum, curr, rev, e, next, w)) {
                is_tip = false;
                break;
            }
            curr = next;
            ++len;
            bases += w;
            mine = mark[curr] == key;
            if (len > max_len + 1 || bases > (long long)max_bases) {
                is_tip = false;
                break;
            }
        }
        if (!mine) {
            c[0] = 1;
        } else {
            cstate[k] = TS_RESOLVED;
            if (is_tip) {
                curr = s;
                for (uint32_t i = 1; i < len; ++i) {
                    uint32_t e, next;
                    int32_t w;
                    if (!tip_step(edges, n_edges, g.fsum, curr, rev, e, next, w)) break;
                    eflag[e] = which;
                    atomicSub(&g.fdeg[curr], 1u);
                    atomicSub(&g.fsum[curr], e);
                    atomicSub(&g.bdeg[next], 1u);
                    atomicSub(&g.bsum[next], e);
                    curr = next;
                }
            }
        }
    }
    block_add<1>(c, unresolved);
}

// (u, v) -> edge id.  The pairs of an edge result are distinct.
__global__ __launch_bounds__(256) void k_tips_insert(const Edge* __restrict__ edges, uint32_t n_edges,
                                                     unsigned long long* __restrict__ tkey, uint32_t* __restrict__ tval,
                                                     uint32_t n_slots) {
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        const Edge ed = edges[e];
        const unsigned long long key = ((unsigned long long)ed.u << 32) | ed.v;
        uint32_t s = edge_slot(ed.u, ed.v, n_slots);
        for (;;) {
            const unsigned long long cur = atomicCAS(&tkey[s], EDGE_EMPTY, key);
            if (cur == EDGE_EMPTY) break;
            if (++s == n_slots) s = 0;
        }
        tval[s] = e;
    }
}

// make_symmetric on the graph the two tip passes left (assembly_graph.py:439-441), one pass; reads eflag only
__global__ __launch_bounds__(256) void k_tips_symmetric(const Edge* __restrict__ edges, uint32_t n_edges,
                                                        const unsigned long long* __restrict__ tkey,
                                                        const uint32_t* __restrict__ tval, uint32_t n_slots,
                                                        const uint8_t* __restrict__ eflag, uint8_t* __restrict__ flags,
                                                        uint8_t* __restrict__ keep, unsigned long long* __restrict__ counters) {
    uint64_t c[3] = {0, 0, 0};
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        uint32_t f = eflag[e];
        if (!f) {
            const Edge ed = edges[e];
            const uint32_t a = ed.v ^ 1u, b = ed.u ^ 1u;
            const unsigned long long key = ((unsigned long long)a << 32) | b;
            uint32_t s = edge_slot(a, b, n_slots);
            for (;;) {
                const unsigned long long cur = tkey[s];
                if (cur == key) {
                    if (eflag[tval[s]]) f = 3;
                    break;
                }
                if (cur == EDGE_EMPTY) {
                    f = 3;
                    break;
                }
                if (++s == n_slots) s = 0;
            }
        }
        flags[e] = (uint8_t)f;
        keep[e] = f == 0;
        c[TC_IN] += f == 1;
        c[TC_OUT] += f == 2;
        c[TC_ASYM] += f == 3;
    }
    block_add<3>(c, counters);
}

__global__ __launch_bounds__(256) void k_tips_alive(const Edge* __restrict__ edges, uint32_t n_edges,
                                                    const uint8_t* __restrict__ keep, uint8_t* __restrict__ alive) {
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        if (!keep[e]) continue;
        alive[edges[e].u] = 1;   // (every writer stores the same byte)
        alive[edges[e].v] = 1;
    }
}

// clean_graph, assembly_graph.py:450-451: a node of the graph without an edge is counted and leaves the node order
__global__ __launch_bounds__(256) void k_tips_nodes(uint32_t n_nodes, const unsigned long long* __restrict__ nrank,
                                                    const uint8_t* __restrict__ alive, unsigned long long* __restrict__ nrank_out,
                                                    unsigned long long* __restrict__ counters) {
    uint64_t c[2] = {0, 0};
    for (uint32_t n = blockIdx.x * blockDim.x + threadIdx.x; n < n_nodes; n += gridDim.x * blockDim.x) {
        const unsigned long long r = nrank[n];
        const bool member = r != NODE_NO_RANK, gone = member && !alive[n];
        nrank_out[n] = gone ? NODE_NO_RANK : r;
        c[0] += member;
        c[1] += gone;
    }
    block_add<2>(c, counters + TC_NODES);
}

}  // namespace po
