// Device side of the diamond-tip removal of `phasm layout` stage 2:
//   remove_diamond_tips                           phasm/assembly_graph.py:721-743, phasm/cli/assembler.py:173
// on an edge result (po_layout_edges, po_layout_reduce, po_layout_tips or po_layout_diamonds itself) in HBM.
//
// The reference visits the end nodes (out-degree 0, in-degree 2 at the start) in the graph's node order.  An end node E
// whose two predecessors are a pred1 (out == 1 and in == 1) and a gt1 (out > 1) is a diamond: E and pred1 leave the graph
// as NODES, which takes three edges out -- the two in-edges of E and the one in-edge (pp, pred1).  Only out-degrees of
// surviving nodes change by that (gt1 and pp lose one each, two when they are one node); the in-degree and the in-edges
// of a surviving node never do, so an end node finds both predecessors as they were.  What changes is their SHAPE: a
// predecessor whose out-degree an earlier diamond took from 2 to 1 is no gt1 any more, and is a pred1 if its in-degree
// is 1 -- the answer depends on the order.  The order is a rank per node (k_layout_node_rank, layout.hip.h); the
// decisions run in ROUNDS that give the sequential answer, as in tips.hip.h:
//   a candidate's FOOTPRINT = its two predecessors a and b and, of each of them with in-degree 1, the one predecessor:
//   at most four nodes, static, and every node the candidate's decision reads or writes
//   k_diamond_mark      every unresolved candidate writes its key (round, rank) into the mark word of its footprint,
//                       atomicMin; later rounds carry smaller keys, so the words need no reset in between
//   k_diamond_resolve   a candidate that finds its own key on all of them is RESOLVED: no unresolved candidate of lower
//                       rank shares a node with it, and a resolved one of higher rank held all of its own marks, so it
//                       shared none either.  It decides as the reference does and, if it is a diamond, flags the three
//                       edges, lowers the two out-degrees and marks E and pred1 removed.
// The lowest unresolved candidate always resolves, so the rounds end.  Candidates that share a predecessor settle one per
// round.  Edge ids without adjacency lists: per node the MIN and MAX id of its in-edges -- the two in-edges at
// in-degree 2, the one in-edge twice at in-degree 1.  Nothing on the out side needs an id.
//   k_diamond_degree / _candidates   degrees, in-edge ids, the candidate list (any order: the rank decides)
//   k_diamond_nodes                  flag byte per edge -> keep byte; a removed node loses its rank, every other node
//                                    keeps it, isolated or not (no clean_graph follows, assembler.py:173-177)
#pragma once

namespace po {

enum { DC_INVALID = 0, DC_CAND = 1, DC_DIAMONDS = 2, DC_NODES = 3, DC_REMOVED = 4, DC_KEPT = 5, DC_N = 6 };
constexpr uint32_t DIAMOND_NO_EDGE = 0xFFFFFFFFu;

__global__ __launch_bounds__(256) void k_diamond_degree(const Edge* __restrict__ edges, uint32_t n_edges, uint32_t n_nodes,
                                                        uint32_t* __restrict__ outdeg, uint32_t* __restrict__ indeg,
                                                        uint32_t* __restrict__ inmin, uint32_t* __restrict__ inmax,
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
        atomicAdd(&indeg[v], 1u);
        atomicMin(&inmin[v], e);
        atomicMax(&inmax[v], e);
    }
    const uint64_t s = wave_sum64(c[0]);
    if (lane_id() == 0 && s) atomicAdd(&counters[DC_INVALID], (unsigned long long)s);
}

// end_nodes = [n for n in g if out_degree(n) == 0 and in_degree(n) == 2] (:722-723); a node without a rank is no node of
// the graph
__global__ __launch_bounds__(256) void k_diamond_candidates(uint32_t n_nodes, const unsigned long long* __restrict__ nrank,
                                                            const uint32_t* __restrict__ outdeg, const uint32_t* __restrict__ indeg,
                                                            uint32_t* __restrict__ cand, uint8_t* __restrict__ cstate,
                                                            uint8_t* __restrict__ removed, unsigned long long* __restrict__ counters) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_nodes) return;
    removed[n] = 0;
    if (nrank[n] == NODE_NO_RANK || outdeg[n] != 0 || indeg[n] != 2) return;
    const uint32_t k = (uint32_t)atomicAdd(&counters[DC_CAND], 1ull);
    cand[k] = n;
    cstate[k] = TS_UNRESOLVED;
}

// The footprint of end node E: f[0], f[1] its predecessors (through the in-edges ea <= eb), f[2], f[3] their single
// predecessors or the predecessor itself again where its in-degree is not 1; epa, epb the in-edge of a resp. b.
struct DiamondFoot {
    uint32_t f[4];
    uint32_t ea, eb, epa, epb;
    bool ok;
};

__device__ inline DiamondFoot diamond_foot(const Edge* __restrict__ edges, uint32_t n_edges, const uint32_t* __restrict__ indeg,
                                           const uint32_t* __restrict__ inmin, const uint32_t* __restrict__ inmax, uint32_t E) {
    DiamondFoot d;
    d.ea = inmin[E];
    d.eb = inmax[E];
    d.epa = d.epb = DIAMOND_NO_EDGE;
    d.ok = d.ea < n_edges && d.eb < n_edges;   // (cannot fail while degree and ids agree; never index on trust)
    d.f[0] = d.f[1] = d.f[2] = d.f[3] = E;
    if (!d.ok) return d;
    const uint32_t a = edges[d.ea].u, b = edges[d.eb].u;
    d.f[0] = d.f[2] = a;
    d.f[1] = d.f[3] = b;
    if (indeg[a] == 1) {
        d.epa = inmin[a];
        if (d.epa < n_edges) d.f[2] = edges[d.epa].u; else d.ok = false;
    }
    if (indeg[b] == 1) {
        d.epb = inmin[b];
        if (d.epb < n_edges) d.f[3] = edges[d.epb].u; else d.ok = false;
    }
    return d;
}

__global__ __launch_bounds__(256) void k_diamond_mark(const Edge* __restrict__ edges, uint32_t n_edges, uint32_t round,
                                                      const uint32_t* __restrict__ cand, const uint8_t* __restrict__ cstate,
                                                      uint32_t n_cand, const unsigned long long* __restrict__ nrank,
                                                      const uint32_t* __restrict__ indeg, const uint32_t* __restrict__ inmin,
                                                      const uint32_t* __restrict__ inmax, unsigned long long* __restrict__ mark) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_cand || cstate[k] != TS_UNRESOLVED) return;
    const uint32_t E = cand[k];
    const unsigned long long key = tip_key(round, nrank[E]);
    const DiamondFoot d = diamond_foot(edges, n_edges, indeg, inmin, inmax, E);
    if (!d.ok) return;
    for (int i = 0; i < 4; ++i) atomicMin(&mark[d.f[i]], key);
}

// remove_diamond_tips for one end node, :727-741.  The out-degrees are read only once every mark is found to be this
// candidate's own: no other candidate of this round writes them then.
__global__ __launch_bounds__(256) void k_diamond_resolve(const Edge* __restrict__ edges, uint32_t n_edges, uint32_t round,
                                                         const uint32_t* __restrict__ cand, uint8_t* __restrict__ cstate,
                                                         uint32_t n_cand, const unsigned long long* __restrict__ nrank,
                                                         uint32_t* outdeg, const uint32_t* __restrict__ indeg,
                                                         const uint32_t* __restrict__ inmin, const uint32_t* __restrict__ inmax,
                                                         const unsigned long long* __restrict__ mark, uint8_t* __restrict__ eflag,
                                                         uint8_t* __restrict__ removed, unsigned long long* __restrict__ unresolved,
                                                         unsigned long long* __restrict__ counters) {
    uint64_t c[1] = {0};   // candidates left unresolved
    uint64_t dm[1] = {0};  // diamonds of this round
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n_cand && cstate[k] == TS_UNRESOLVED) {
        const uint32_t E = cand[k];
        const unsigned long long key = tip_key(round, nrank[E]);
        const DiamondFoot d = diamond_foot(edges, n_edges, indeg, inmin, inmax, E);
        bool mine = true;
        for (int i = 0; i < 4; ++i) mine = mine && mark[d.f[i]] == key;
        if (!d.ok) {
            cstate[k] = TS_RESOLVED;   // (no footprint to decide on: nothing happens, and the rounds must end)
        } else if (!mine) {
            c[0] = 1;
        } else {
            cstate[k] = TS_RESOLVED;
            const uint32_t a = d.f[0], b = d.f[1];
            const uint32_t oa = outdeg[a], ob = outdeg[b];
            const bool a1 = oa == 1 && d.epa != DIAMOND_NO_EDGE, b1 = ob == 1 && d.epb != DIAMOND_NO_EDGE;
            // one pred1 and one gt1 (a node cannot be both; with two of a kind the other kind is missing)
            if ((a1 && ob > 1) || (b1 && oa > 1)) {
                const uint32_t pred1 = a1 ? a : b, gt1 = a1 ? b : a, pp = a1 ? d.f[2] : d.f[3], ep = a1 ? d.epa : d.epb;
                eflag[d.ea] = 1;
                eflag[d.eb] = 1;
                eflag[ep] = 2;
                atomicSub(&outdeg[gt1], 1u);
                atomicSub(&outdeg[pp], 1u);
                removed[E] = 1;
                removed[pred1] = 1;
                dm[0] = 1;
            }
        }
    }
    block_add<1>(c, unresolved);
    block_add<1>(dm, counters + DC_DIAMONDS);
}

// keep byte per edge; a removed node leaves the node order, every other node stays in it
__global__ __launch_bounds__(256) void k_diamond_nodes(uint32_t n_edges, uint32_t n_nodes, const uint8_t* __restrict__ eflag,
                                                       uint8_t* __restrict__ keep, const unsigned long long* __restrict__ nrank,
                                                       const uint8_t* __restrict__ removed, unsigned long long* __restrict__ nrank_out,
                                                       unsigned long long* __restrict__ counters) {
    uint64_t c[3] = {0, 0, 0};
    const uint32_t stride = gridDim.x * blockDim.x, t = blockIdx.x * blockDim.x + threadIdx.x;
    for (uint32_t n = t; n < n_nodes; n += stride) {
        const unsigned long long r = nrank[n];
        const bool member = r != NODE_NO_RANK, gone = member && removed[n];
        nrank_out[n] = gone ? NODE_NO_RANK : r;
        c[0] += member;
        c[1] += gone;
    }
    for (uint32_t e = t; e < n_edges; e += stride) {
        const uint8_t k = eflag[e] == 0;
        keep[e] = k;
        c[2] += k;
    }
    block_add<3>(c, counters + DC_NODES);
}

}  // namespace po
