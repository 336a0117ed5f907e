// Device side of the merging of unambiguous paths of `phasm layout` stage 2:
//   merge_unambiguous_paths                       phasm/assembly_graph.py:456-541, phasm/cli/assembler.py:184-186
// on an edge result (po_layout_edges, _reduce, _tips or _diamonds) in HBM.
//
// link(u) = v iff u has one out-edge, into v, and v has one in-edge.  Links form disjoint paths and cycles; a HEAD is a
// node with a link out and none in, its path the head followed by its links.  Every path becomes one merged node,
// numbered by the rank of its head in the node order; nodes on link cycles stay as they are.  Degrees never change, so
// nothing here depends on an order but the numbering.
//   k_merge_degree / _links   degrees and the id of the one out- / in-edge (the MIN id: the only one at degree 1), then
//                             link, back (the link into a node) and the compacted heads with their rank words
//   k_merge_jump              list ranking by pointer jumping along `back`, one launch per round, ping-pong buffers: per
//                             node (jb, hops, wsum), a root (no link in) points at itself with hops = wsum = 0, so
//                             hops += hops[jb]; wsum += wsum[jb]; jb = jb[jb] is the whole round.  After r rounds a node
//                             d links behind its head holds min(d, 2^r) hops.  A round counts the nodes that REACHED a
//                             root in it; as every distance 1..d_max occurs on a path, a round that counts none ends the
//                             ranking.  Nodes of a cycle never reach a root.  No loop follows links: the host bounds the rounds.
//   k_merge_tails             path length and weight sum at the head (written by the path's one last node), counters
//   k_merge_bitonic           sort of (rank word, head) -- one launch per compare-exchange step, padded to a power of two
//   k_merge_number            k = position: path k of the head, nodes and weight sum of path k
//   k_merge_tables            member / prefix tables at offset[k] + hops, length[k], (path, pos) per node
//   k_merge_ranks             the node order of the result: path nodes leave, merged node k ranks behind every old node
//   k_merge_edges             flag byte per edge, the kept edges renamed (merged node k = n_nodes + k) and re-weighted
#pragma once

namespace po {

enum { MC_INVALID = 0, MC_MAXRANK = 1, MC_HEADS = 2, MC_NODES = 3, MC_LINKED = 4, MC_MERGED = 5, MC_CYCLE = 6, MC_MAXPATH = 7,
       MC_SELF = 8, MC_OVERFLOW = 9, MC_KEPT = 10, MC_N = 11 };   // (NODES/LINKED, MERGED/CYCLE, SELF/OVERFLOW/KEPT: one block_add each)
constexpr uint32_t MERGE_NONE = 0xFFFFFFFFu;

// ---- the host's schedule of the rounds and of the sort: run_merge (c_api.hip) and the host emulation of the tests
// (tools/merge_host_emu.cpp) both launch by these ----------------------------------------------------------------------
constexpr uint32_t MERGE_BATCH = 8;   // pointer-jumping rounds per readback

// ceil(log2(n_nodes)) + 1: a node sits fewer than n_nodes links behind its head
inline uint32_t merge_round_cap(uint64_t n_nodes) {
    uint32_t cap = 1;
    while ((1ull << (cap - 1)) < n_nodes) ++cap;
    return cap;
}

// The words of one batch: word j = nodes that reached a root in round j.  Counts the rounds up to and including the first
// that brought none; true when that round was met.
inline bool merge_rounds_done(const volatile uint64_t* words, uint32_t batch, uint32_t& rounds) {
    for (uint32_t j = 0; j < batch; ++j) {
        ++rounds;
        if (words[j] == 0) return true;
    }
    return false;
}

// launch i reads triple (i & 1) and writes the other: after `launched` launches the result is in triple (launched & 1)
inline int merge_final_buffer(uint32_t launched) { return (int)(launched & 1); }

inline uint32_t merge_sort_pad(uint32_t n_heads) {
    uint32_t pad = 1;
    while (pad < n_heads) pad <<= 1;
    return pad;
}

// the compare-exchange steps (j, k) of a bitonic sort of merge_sort_pad(n_heads) keys, in launch order
template <class F>
inline void merge_sort_steps(uint32_t n_heads, F&& step) {
    const uint32_t pad = merge_sort_pad(n_heads);
    for (uint32_t k = 2; k <= pad && n_heads > 1; k <<= 1)
        for (uint32_t j = k >> 1; j; j >>= 1) step(j, k);
}

__device__ inline unsigned long long merge_wave_max(unsigned long long v) {
    for (int off = WAVE >> 1; off; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off, WAVE);
        v = o > v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(256) void k_merge_degree(const Edge* __restrict__ edges, uint32_t n_edges, uint32_t n_nodes,
                                                      uint32_t* __restrict__ outdeg, uint32_t* __restrict__ indeg,
                                                      uint32_t* __restrict__ oute, uint32_t* __restrict__ ine,
                                                      unsigned long long* __restrict__ counters) {
    uint64_t c[1] = {0};
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        const uint32_t u = edges[e].u, v = edges[e].v;
        if (u >= n_nodes || v >= n_nodes) {
            c[0] += 1;
            continue;
        }
        atomicAdd(&outdeg[u], 1u);
        atomicAdd(&indeg[v], 1u);
        atomicMin(&oute[u], e);
        atomicMin(&ine[v], e);
    }
    const uint64_t s = wave_sum64(c[0]);
    if (lane_id() == 0 && s) atomicAdd(&counters[MC_INVALID], (unsigned long long)s);
}

// link, back and the start of the ranking per node; the heads, compacted in any order (the sort orders them)
__global__ __launch_bounds__(256) void k_merge_links(const Edge* __restrict__ edges, uint32_t n_edges, uint32_t n_nodes,
                                                     const unsigned long long* __restrict__ nrank,
                                                     const uint32_t* __restrict__ outdeg, const uint32_t* __restrict__ indeg,
                                                     const uint32_t* __restrict__ oute, const uint32_t* __restrict__ ine,
                                                     uint32_t* __restrict__ link, uint32_t* __restrict__ back,
                                                     uint32_t* __restrict__ jb, uint32_t* __restrict__ hops,
                                                     unsigned long long* __restrict__ wsum, uint32_t* __restrict__ hlen,
                                                     unsigned long long* __restrict__ hkey, uint32_t* __restrict__ hval,
                                                     unsigned long long* __restrict__ counters) {
    uint64_t c[2] = {0, 0};   // nodes in the order, nodes with a link into them
    unsigned long long top = 0;
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n < n_nodes) {
        uint32_t l = MERGE_NONE, b = MERGE_NONE;
        long long w = 0;
        if (outdeg[n] == 1) {
            const uint32_t e = oute[n];
            if (e < n_edges && indeg[edges[e].v] == 1) l = edges[e].v;   // (never index on trust)
        }
        if (indeg[n] == 1) {
            const uint32_t e = ine[n];
            if (e < n_edges && outdeg[edges[e].u] == 1) {
                b = edges[e].u;
                w = edges[e].weight;
            }
        }
        link[n] = l;
        back[n] = b;
        jb[n] = b == MERGE_NONE ? n : b;
        hops[n] = b != MERGE_NONE;
        wsum[n] = (unsigned long long)w;
        hlen[n] = 0;
        const unsigned long long r = nrank[n];
        if (r != NODE_NO_RANK) {
            c[0] = 1;
            top = r;
        }
        c[1] = b != MERGE_NONE;
        if (l != MERGE_NONE && b == MERGE_NONE) {
            const uint32_t k = (uint32_t)atomicAdd(&counters[MC_HEADS], 1ull);
            hkey[k] = r;
            hval[k] = n;
        }
    }
    top = merge_wave_max(top);
    if (lane_id() == 0 && top) atomicMax(&counters[MC_MAXRANK], top);
    block_add<2>(c, counters + MC_NODES);
}

// one round of pointer jumping: reads the `in` triple of two nodes, writes the `out` triple of its own
__global__ __launch_bounds__(256) void k_merge_jump(uint32_t n_nodes, const uint32_t* __restrict__ back,
                                                    const uint32_t* __restrict__ jb_in, const uint32_t* __restrict__ hops_in,
                                                    const unsigned long long* __restrict__ ws_in, uint32_t* __restrict__ jb_out,
                                                    uint32_t* __restrict__ hops_out, unsigned long long* __restrict__ ws_out,
                                                    unsigned long long* __restrict__ reached) {
    uint64_t c[1] = {0};
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n < n_nodes) {
        const uint32_t j = jb_in[n];
        const uint32_t jj = jb_in[j];
        jb_out[n] = jj;
        hops_out[n] = hops_in[n] + hops_in[j];
        ws_out[n] = ws_in[n] + ws_in[j];
        c[0] = back[j] != MERGE_NONE && back[jj] == MERGE_NONE;
    }
    block_add<1>(c, reached);
}

// A node with a link into it whose jb is a root has reached its head.  The one such node without a link out is the path's
// last: it knows the path's node count and weight sum.
__global__ __launch_bounds__(256) void k_merge_tails(uint32_t n_nodes, const uint32_t* __restrict__ link,
                                                     const uint32_t* __restrict__ back, const uint32_t* __restrict__ jb,
                                                     const uint32_t* __restrict__ hops, const unsigned long long* __restrict__ wsum,
                                                     uint32_t* __restrict__ hlen, unsigned long long* __restrict__ hsum,
                                                     unsigned long long* __restrict__ counters) {
    uint64_t c[2] = {0, 0};   // nodes on paths, nodes on cycles
    unsigned long long longest = 0;
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n < n_nodes) {
        const uint32_t l = link[n], b = back[n];
        if (b == MERGE_NONE) {
            c[0] = l != MERGE_NONE;
        } else {
            const uint32_t r = jb[n];
            if (back[r] == MERGE_NONE) {
                c[0] = 1;
                if (l == MERGE_NONE) {
                    hlen[r] = hops[n] + 1;
                    hsum[r] = wsum[n];
                    longest = (unsigned long long)hops[n] + 1;
                }
            } else {
                c[1] = l != MERGE_NONE;
            }
        }
    }
    longest = merge_wave_max(longest);
    if (lane_id() == 0 && longest) atomicMax(&counters[MC_MAXPATH], longest);
    block_add<2>(c, counters + MC_MERGED);
}

// one compare-exchange step of a bitonic sort of n_pad = 2^p (key, value) pairs: partner distance j inside runs of k
__global__ __launch_bounds__(256) void k_merge_bitonic(unsigned long long* __restrict__ key, uint32_t* __restrict__ val,
                                                       uint32_t n_pad, uint32_t j, uint32_t k) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t p = i ^ j;
    if (i >= n_pad || p <= i || p >= n_pad) return;
    const unsigned long long a = key[i], b = key[p];
    const bool up = (i & k) == 0;
    if ((a > b) == up && a != b) {
        key[i] = b;
        key[p] = a;
        const uint32_t va = val[i], vb = val[p];
        val[i] = vb;
        val[p] = va;
    }
}

__global__ __launch_bounds__(256) void k_merge_number(uint32_t n_paths, uint32_t n_nodes, const uint32_t* __restrict__ hval,
                                                      const uint32_t* __restrict__ hlen, const unsigned long long* __restrict__ hsum,
                                                      uint32_t* __restrict__ pathk, uint32_t* __restrict__ lens,
                                                      long long* __restrict__ psum) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_paths) return;
    const uint32_t h = hval[k];
    if (h >= n_nodes) return;
    pathk[h] = k;
    lens[k] = hlen[h];
    psum[k] = (long long)hsum[h];
}

__global__ __launch_bounds__(256) void k_merge_tables(const Edge* __restrict__ edges, uint32_t n_edges, uint32_t n_nodes,
                                                      const uint32_t* __restrict__ len, const uint32_t* __restrict__ link,
                                                      const uint32_t* __restrict__ back, const uint32_t* __restrict__ jb,
                                                      const uint32_t* __restrict__ hops, const unsigned long long* __restrict__ wsum,
                                                      const uint32_t* __restrict__ oute, const uint32_t* __restrict__ pathk,
                                                      const uint32_t* __restrict__ off, uint32_t n_paths, uint32_t n_members,
                                                      uint32_t* __restrict__ member, int32_t* __restrict__ prefix,
                                                      long long* __restrict__ length, uint32_t* __restrict__ npath,
                                                      uint32_t* __restrict__ npos) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_nodes) return;
    const uint32_t l = link[n], b = back[n];
    const uint32_t r = b == MERGE_NONE ? n : jb[n];
    const bool on = b == MERGE_NONE ? l != MERGE_NONE : back[r] == MERGE_NONE;
    uint32_t k = MERGE_NONE, pos = 0;
    if (on) {
        k = pathk[r];
        pos = b == MERGE_NONE ? 0u : hops[n];
        const uint32_t at = k < n_paths ? off[k] + pos : n_members;
        if (at < n_members) {
            member[at] = n;
            const uint32_t e = oute[n];
            prefix[at] = l != MERGE_NONE && e < n_edges ? edges[e].weight : 0;
            if (l == MERGE_NONE) length[k] = (long long)wsum[n] + (long long)len[n];
        } else {
            k = MERGE_NONE;   // (cannot happen while the lengths and the offsets agree)
        }
    }
    npath[n] = k;
    npos[n] = k == MERGE_NONE ? 0u : pos;
}

__global__ __launch_bounds__(256) void k_merge_ranks(uint32_t n_nodes, uint32_t n_paths, const unsigned long long* __restrict__ nrank,
                                                     const uint32_t* __restrict__ npath, const unsigned long long* __restrict__ counters,
                                                     unsigned long long* __restrict__ nrank_out) {
    const uint32_t stride = gridDim.x * blockDim.x, t = blockIdx.x * blockDim.x + threadIdx.x;
    for (uint32_t n = t; n < n_nodes; n += stride) nrank_out[n] = npath[n] != MERGE_NONE ? NODE_NO_RANK : nrank[n];
    const unsigned long long base = counters[MC_MAXRANK] + 1;
    for (uint32_t k = t; k < n_paths; k += stride) nrank_out[(size_t)n_nodes + k] = base + k;
}

// 0 kept as it is, 1 path edge, 2 kept with a renamed end or a raised weight.  An end on a path is the path's last node
// as u (every other path node has one out-edge, the link) and its head as v.
__global__ __launch_bounds__(256) void k_merge_edges(const Edge* __restrict__ edges, uint32_t n_edges, uint32_t n_nodes,
                                                     const uint32_t* __restrict__ link, const uint32_t* __restrict__ npath,
                                                     const long long* __restrict__ psum, Edge* __restrict__ renamed,
                                                     uint8_t* __restrict__ eflag, uint8_t* __restrict__ keep,
                                                     unsigned long long* __restrict__ counters) {
    uint64_t c[3] = {0, 0, 0};   // self-loops of merged nodes, weights that do not fit, edges kept
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        Edge x = edges[e];
        const uint32_t pu = npath[x.u], pv = npath[x.v];
        if (pu != MERGE_NONE && link[x.u] == x.v) {
            eflag[e] = 1;
            keep[e] = 0;
            renamed[e] = x;
            continue;
        }
        if (pu != MERGE_NONE) {
            const long long w = (long long)x.weight + psum[pu];
            if (w > 2147483647ll || w < -2147483648ll) c[1] += 1; else x.weight = (int32_t)w;
            x.u = n_nodes + pu;
            c[0] += pu == pv;
        }
        if (pv != MERGE_NONE) x.v = n_nodes + pv;
        eflag[e] = (pu != MERGE_NONE || pv != MERGE_NONE) ? 2 : 0;
        keep[e] = 1;
        renamed[e] = x;
        c[2] += 1;
    }
    block_add<3>(c, counters + MC_SELF);
}

}  // namespace po
