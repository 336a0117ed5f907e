// Device side of the superbubbles of the WHOLE graph, the cyclic partitions included:
//   what find_superbubbles reaches through graph_to_dag                  phasm/bubbles.py:104-171, 397-445
// on a graph result in HBM, by ROOT SPLITTING.  po_layout_superbubbles_all runs the SCC stage of partition.hip.h and the
// stage of superbubbles.hip.h unchanged, on a FLAT graph that the kernels here build; nothing of either is copied.
//
// SPLITTING a rank x: x_out keeps the rank x and all out-edges (a source), x_in = n_order + (number of split ranks below
// x) takes ALL in-edges (a sink).  The flat graph has n_order + n_split ranks and the edges of the graph, heads remapped.
//   k_cy_flat / k_cy_ranks                     behind a prefix sum over the split bytes: the flat edge list; the node and
//                                              the original rank of every flat rank
//   k_cy_choose / k_cy_apply                   behind the SCC stage on the flat graph: per non-singleton SCC the lowest
//                                              rank with R_IN, with RE_OUT, of all (atomicMin over the flagged ranks), then
//                                              the split byte of the first of the three that exists -- for a ROOTLESS SCC
//                                              (neither flag on any member: a whole weak component) the root this run was
//                                              given.  Levels, until the SCC stage finds singletons only
//   k_cy_level0 / k_cy_uncertain               level 0: the SCC of the graph itself per rank, "not a singleton";
//                                              level 1: an SCC that still holds a cycle is not CERTIFIED by its root
//   k_cy_seed_edges / k_cy_seed_ranks          before the discard rounds of the stage: a pair whose ends are the two copies
//                                              of one rank, and a pair (s, t) with an edge t -> s, are dead
//   k_cy_merge                                 the run's pairs, holders and totals into the merged words by original rank:
//                                              pairs by union, the holder with the smallest n_inside
//   k_cy_bfs_init / k_cy_bfs_round / k_cy_bfs_parents
//                                              one shortest cycle through the root of every uncertified rootless SCC:
//                                              distances by atomicMin per edge in rounds, then the lowest-ranked parent one
//                                              step nearer; the host walks the parents back
//   k_cy_loops / k_cy_final                    the outputs by rank, the root bytes of the table, the counts
// Words are WRITTEN by atomicMin or by the one thread that owns the rank, bytes by plain stores of one value; a plain load
// may see an older word, which is a higher one: a round then does less, the round that ends a loop wrote nothing.
// Integer atomics only: every output is the same on every run.
#pragma once

namespace po {

enum { YC_ROOTLESS = 0, YC_NESTED = 1, YC_CYCLIC = 2, YC_FILTERED = 3, YC_BAD = 4, YC_N = 5 };

__global__ __launch_bounds__(256) void k_cy_flat(const EdgeRanks* __restrict__ er, uint32_t n_edges, uint32_t n_order,
                                                 const uint8_t* __restrict__ split, const uint32_t* __restrict__ sidx,
                                                 uint32_t n_split, EdgeRanks* __restrict__ flat) {
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        EdgeRanks x = er[e];
        if (x.ru >= n_order || x.rv >= n_order) x = EdgeRanks{CC_NONE, CC_NONE};   // (every later kernel skips it)
        else if (split[x.rv]) x.rv = sidx[x.rv] < n_split ? n_order + sidx[x.rv] : CC_NONE;
        flat[e] = x;
    }
}

__global__ __launch_bounds__(256) void k_cy_ranks(uint32_t n_order, const uint32_t* __restrict__ node_at,
                                                  const uint8_t* __restrict__ split, const uint32_t* __restrict__ sidx,
                                                  uint32_t n_split, uint32_t* __restrict__ flat_node, uint32_t* __restrict__ orig) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        flat_node[r] = node_at[r];
        orig[r] = r;
        if (!split[r]) continue;
        const uint32_t i = sidx[r];
        if (i >= n_split) continue;   // (cannot happen: the prefix sum counted this rank)
        flat_node[n_order + i] = node_at[r];
        orig[n_order + i] = r;
    }
}

// per rank of a non-singleton SCC of the flat graph (an unsplit rank below n_order: a copy is an SCC of its own)
__global__ __launch_bounds__(256) void k_cy_choose(uint32_t n_order, uint32_t n_scc, const uint32_t* __restrict__ node_scc,
                                                   const Scc* __restrict__ table, const uint8_t* __restrict__ flags,
                                                   uint32_t* __restrict__ best_in, uint32_t* __restrict__ best_out,
                                                   uint32_t* __restrict__ best_low) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        const uint32_t c = node_scc[r];
        if (c >= n_scc || table[c].n_nodes < 2) continue;
        const uint32_t f = flags[r];
        if (f & SF_R_IN) atomicMin(&best_in[c], r);
        if (f & SF_RE_OUT) atomicMin(&best_out[c], r);
        atomicMin(&best_low[c], r);
    }
}

// per SCC: the split byte of its root.  root_of (level 0 only, else null): the root of a rootless SCC, by its lowest rank;
// rootless (level 0 only, else null): the byte of that lowest rank
__global__ __launch_bounds__(256) void k_cy_apply(uint32_t n_order, uint32_t n_scc, const Scc* __restrict__ table,
                                                  const uint32_t* __restrict__ best_in, const uint32_t* __restrict__ best_out,
                                                  const uint32_t* __restrict__ best_low, const uint32_t* __restrict__ root_of,
                                                  uint8_t* __restrict__ rootless, uint8_t* __restrict__ split,
                                                  unsigned long long* __restrict__ counters) {
    uint64_t c2[2] = {0, 0};   // rootless SCCs, roots that cannot be
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < n_scc; c += gridDim.x * blockDim.x) {
        if (table[c].n_nodes < 2) continue;
        const uint32_t low = best_low[c];
        uint32_t x = best_in[c] != CC_NONE ? best_in[c] : best_out[c];
        if (x == CC_NONE) {
            x = low;
            if (low < n_order && rootless) {
                rootless[low] = 1;
                ++c2[0];
            }
            if (low < n_order && root_of) x = root_of[low];
        }
        if (x < n_order) split[x] = 1;
        else ++c2[1];
    }
    const uint64_t a = wave_sum64(c2[0]), b = wave_sum64(c2[1]);
    if (lane_id() == 0 && a) atomicAdd(&counters[YC_ROOTLESS], (unsigned long long)a);
    if (lane_id() == 0 && b) atomicAdd(&counters[YC_BAD], (unsigned long long)b);
}

__global__ __launch_bounds__(256) void k_cy_level0(uint32_t n_order, uint32_t n_scc, const uint32_t* __restrict__ node_scc,
                                                   const Scc* __restrict__ table, const uint32_t* __restrict__ scc,
                                                   uint32_t* __restrict__ scc0, uint8_t* __restrict__ cyclic0) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        const uint32_t c = node_scc[r];
        scc0[r] = scc[r];
        cyclic0[r] = c < n_scc && table[c].n_nodes > 1;
    }
}

__global__ __launch_bounds__(256) void k_cy_uncertain(uint32_t n_order, uint32_t n_scc, const uint32_t* __restrict__ node_scc,
                                                      const Scc* __restrict__ table, const uint32_t* __restrict__ scc0,
                                                      uint8_t* __restrict__ uncertain) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        const uint32_t c = node_scc[r], low = scc0[r];
        if (c < n_scc && table[c].n_nodes > 1 && low < n_order) uncertain[low] = 1;   // (every writer stores the same value)
    }
}

// per edge (u, v) of the graph: the pair (v, t) that v_out enters with t a copy of u has the edge t -> s
__global__ __launch_bounds__(256) void k_cy_seed_edges(const EdgeRanks* __restrict__ er, uint32_t n_edges, uint32_t n_order,
                                                       uint32_t n_flat, const uint32_t* __restrict__ exit_of,
                                                       const uint32_t* __restrict__ orig, uint8_t* __restrict__ filtered) {
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        const EdgeRanks x = er[e];
        if (x.ru >= n_order || x.rv >= n_order || x.ru == x.rv) continue;
        const uint32_t t = exit_of[x.rv];
        if (t < n_flat && orig[t] == x.ru) filtered[x.rv] = 1;
    }
}

__global__ __launch_bounds__(256) void k_cy_seed_ranks(uint32_t n_order, uint32_t n_flat, const uint32_t* __restrict__ exit_of,
                                                       const uint32_t* __restrict__ orig, const uint8_t* __restrict__ filtered,
                                                       uint8_t* __restrict__ dead, uint8_t* __restrict__ m_filtered) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        const uint32_t t = exit_of[r];
        if (t >= n_flat) continue;
        if (orig[t] == r) dead[r] = 1;   // (x_out, x_in)
        if (filtered[r]) {
            dead[r] = 1;
            m_filtered[r] = 1;
        }
    }
}

// behind k_sb_sum: `root` = enters a surviving bubble, `inside` = the holder, `total` = n_inside, all by flat rank.  An
// entrance and a holder are ranks below n_order (a copy is a sink); only an exit can be a copy.
__global__ __launch_bounds__(256) void k_cy_merge(uint32_t n_order, uint32_t n_flat, const uint32_t* __restrict__ orig,
                                                  const uint8_t* __restrict__ root, const uint32_t* __restrict__ exit_of,
                                                  const uint32_t* __restrict__ inside, const uint32_t* __restrict__ total,
                                                  uint32_t* __restrict__ m_exit, uint32_t* __restrict__ m_inside,
                                                  uint32_t* __restrict__ m_size, uint32_t* __restrict__ m_total,
                                                  uint8_t* __restrict__ m_is_exit) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        const uint32_t t = exit_of[r];
        if (root[r] && t < n_flat && orig[t] < n_order) {
            m_exit[r] = orig[t];
            m_total[r] = total[r];
            m_is_exit[orig[t]] = 1;   // (every writer stores the same value)
        }
        const uint32_t holder = inside[r];
        if (holder < n_order && total[holder] < m_size[r]) {
            m_inside[r] = holder;
            m_size[r] = total[holder];
        }
    }
}

__global__ __launch_bounds__(256) void k_cy_bfs_init(uint32_t n_order, const uint8_t* __restrict__ rootless,
                                                     const uint8_t* __restrict__ uncertain, uint8_t* __restrict__ is_root,
                                                     uint32_t* __restrict__ dist, uint32_t* __restrict__ par, uint32_t* __restrict__ din,
                                                     uint32_t* __restrict__ pin) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        const bool root = rootless[r] && uncertain[r];
        is_root[r] = root;
        dist[r] = root ? 0u : CC_NONE;
        par[r] = din[r] = pin[r] = CC_NONE;
    }
}

// an edge into a root reaches its `in` copy (din), every other edge the rank itself (dist)
__global__ __launch_bounds__(256) void k_cy_bfs_round(const EdgeRanks* __restrict__ er, uint32_t n_edges, uint32_t n_order,
                                                      const uint8_t* __restrict__ is_root, uint32_t* __restrict__ dist,
                                                      uint32_t* __restrict__ din, unsigned long long* __restrict__ changed) {
    uint64_t c = 0;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        const EdgeRanks x = er[e];
        if (x.ru >= n_order || x.rv >= n_order) continue;
        const uint32_t du = dist[x.ru];
        if (du == CC_NONE) continue;
        uint32_t* const w = is_root[x.rv] ? &din[x.rv] : &dist[x.rv];
        if (du + 1 < *w) c += atomicMin(w, du + 1) > du + 1;
    }
    const uint64_t s = wave_sum64(c);
    if (lane_id() == 0 && s) atomicAdd(changed, (unsigned long long)s);
}

__global__ __launch_bounds__(256) void k_cy_bfs_parents(const EdgeRanks* __restrict__ er, uint32_t n_edges, uint32_t n_order,
                                                        const uint8_t* __restrict__ is_root, const uint32_t* __restrict__ dist,
                                                        const uint32_t* __restrict__ din, uint32_t* __restrict__ par,
                                                        uint32_t* __restrict__ pin) {
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        const EdgeRanks x = er[e];
        if (x.ru >= n_order || x.rv >= n_order) continue;
        const uint32_t du = dist[x.ru];
        if (du == CC_NONE) continue;
        if (is_root[x.rv]) {
            if (din[x.rv] == du + 1) atomicMin(&pin[x.rv], x.ru);
        } else if (dist[x.rv] == du + 1) {
            atomicMin(&par[x.rv], x.ru);
        }
    }
}

__global__ __launch_bounds__(256) void k_cy_loops(const EdgeRanks* __restrict__ er, uint32_t n_edges, uint32_t n_order,
                                                  uint8_t* __restrict__ loop) {
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        const EdgeRanks x = er[e];
        if (x.ru < n_order && x.ru == x.rv) loop[x.ru] = 1;
    }
}

__global__ __launch_bounds__(256) void k_cy_final(uint32_t n_order, const uint32_t* __restrict__ node_at,
                                                  const uint32_t* __restrict__ m_exit, const uint32_t* __restrict__ m_inside,
                                                  const uint8_t* __restrict__ m_is_exit, const uint8_t* __restrict__ loop,
                                                  const uint8_t* __restrict__ m_filtered, const uint8_t* __restrict__ cyclic0,
                                                  uint8_t* __restrict__ root, uint32_t* __restrict__ exit_out,
                                                  uint32_t* __restrict__ inside_out, uint8_t* __restrict__ flags_out,
                                                  unsigned long long* __restrict__ counters) {
    uint64_t c[3] = {0, 0, 0};   // nested, in a non-singleton SCC, pairs dropped for an edge t -> s
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        const uint32_t t = m_exit[r], in = m_inside[r];
        const bool enters = t < n_order, held = in < n_order;
        uint32_t f = loop[r] ? SB_SELF_LOOP : 0u;
        if (enters) f |= SB_ENTRANCE | (held ? SB_NESTED : 0u);
        if (m_is_exit[r]) f |= SB_EXIT;
        root[r] = enters;
        exit_out[r] = enters ? node_at[t] : CC_NONE;
        inside_out[r] = held ? node_at[in] : CC_NONE;
        flags_out[r] = (uint8_t)f;
        c[0] += enters && held;
        c[1] += enters && cyclic0[r];
        c[2] += m_filtered[r] != 0;
    }
    block_add<3>(c, counters + YC_NESTED);
}
static_assert(YC_CYCLIC == YC_NESTED + 1 && YC_FILTERED == YC_NESTED + 2, "k_cy_final adds the three in one go");

}  // namespace po
