// Device side of the superbubbles of the acyclic partitions inside `phasm chain`:
//   SuperBubbleFinderDAG(partition)                           phasm/bubbles.py:174-381, called from bubbles.py:411-414
// on a graph result in HBM, behind the SCC stage of partition.hip.h (po_layout_superbubbles runs it first and works on its
// words: the SCC, the class byte of every edge, the flag byte of every rank).
//
// The scheme works on RANKS.  A rank is REAL iff its SCC is a singleton.  D = the class-1 edges with ru != rv (a DAG: every
// real rank is an SCC of its own); a class-1 self-loop only marks its rank.  A real rank is a SOURCE iff it has R_IN or no
// edge of D into it, a SINK iff it has RE_OUT or no edge of D out of it: one virtual root above all sources and one virtual
// sink below all sinks, both named by the rank n_order.
//   k_sb_init / k_sb_degrees / k_sb_fill       the work word per rank, the in- and out-degree in D; behind two prefix sums
//                                              the parents and the children of every rank as lists (filled through an
//                                              atomic cursor: the order inside a list differs from run to run, nothing that
//                                              is computed from a list does)
//   k_sb_nodes                                 sources and sinks; level 1 on every real rank, forward and backward
//   k_sb_level                                 per edge of D: atomicMax(&lvl_f[rv], lvl_f[ru] + 1), atomicMax(&lvl_b[ru],
//                                              lvl_b[rv] + 1).  Rounds, until one raises nothing: the longest-path levels
//   k_sb_tree                                  one launch per level, ascending: a rank of that level folds the lowest
//                                              common ancestor over its neighbours on the root's side (a source starts from
//                                              the root) -- its immediate dominator -- and takes depth = depth[idom] + 1.
//                                              Everything it reads was written by a launch before it.  The walk of lca()
//                                              along the two chains is the one loop along a tree path: bounded by twice the
//                                              level, counted as an error beyond.  Forward for idom, backward for ipdom
//   k_sb_pairs                                 exit[s] = t iff t = ipdom[s] is real and idom[t] == s
//   k_sb_encl                                  one launch per forward level: encl[v] = idom[v] if that is an entrance whose
//                                              exit is not v, else encl[idom[v]]: the innermost bubble that holds v strictly
//   k_sb_dead_init / k_sb_dead_round           a self-loop discards the bubble its rank enters, the one it exits and the
//                                              one that holds it; rounds: a discarded bubble discards encl[its entrance],
//                                              until a round discards nothing
//   k_sb_label                                 per rank: the outputs, the survivors' root bytes, 1 into n_inside of the
//                                              bubble that holds it
//   k_sb_sum                                   one launch per forward level, descending: a surviving nested bubble adds
//                                              its n_inside to the bubble that holds its entrance
//   k_sb_table                                 behind a prefix sum over the survivors: the table in entrance-rank order
// Level words are READ with plain loads, which may see a word as it was earlier in the same launch: an older level is a
// lower one, so a round only does less with it; the round that ends the loop wrote nothing.  The dead bytes likewise: an
// older byte is 0 and the 1 is stored again.  Levels are WRITTEN by atomicMax only, bytes by plain stores of one value.
// Integer atomics only: every output is the same on every run.
#pragma once

namespace po {

enum { BC_LOOPS = 0, BC_R_EDGES = 1, BC_RE_EDGES = 2, BC_LEVF = 3, BC_LEVB = 4, BC_WALK = 5, BC_NESTED = 6, BC_DISCARDED = 7, BC_REAL = 8,
       BC_DEDGES = 9, BC_N = 10 };

enum : uint32_t { SBW_REAL = 1, SBW_LOOP = 2, SBW_SOURCE = 4, SBW_SINK = 8 };
enum : uint32_t { SB_ENTRANCE = 1, SB_EXIT = 2, SB_NESTED = 4, SB_SELF_LOOP = 8 };   // (PO_SB_* of the header)

struct Bubble {
    uint32_t entrance, exit, n_inside, nested;
};

// the lowest common ancestor of a and b in the tree of `idom` (the root is the rank n_order, its own parent, depth 0)
__device__ inline uint32_t sb_lca(uint32_t a, uint32_t b, const uint32_t* idom, const uint32_t* depth, uint32_t n_order, uint32_t cap,
                                  bool& failed) {
    for (uint32_t step = 0; a != b; ++step) {
        if (step > cap || a > n_order || b > n_order) {
            failed = true;
            return n_order;
        }
        if (depth[a] >= depth[b]) a = idom[a];
        else b = idom[b];
    }
    return a;
}

__global__ __launch_bounds__(256) void k_sb_init(uint32_t n_order, uint32_t n_scc, const uint32_t* __restrict__ node_scc,
                                                 const Scc* __restrict__ table, uint32_t* __restrict__ w, uint32_t* __restrict__ cin,
                                                 uint32_t* __restrict__ cout, uint32_t* __restrict__ idom, uint32_t* __restrict__ ipdom,
                                                 uint32_t* __restrict__ depth, uint32_t* __restrict__ exit_of, uint32_t* __restrict__ encl,
                                                 uint32_t* __restrict__ total, uint8_t* __restrict__ dead) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r <= n_order; r += gridDim.x * blockDim.x) {
        idom[r] = ipdom[r] = r == n_order ? n_order : CC_NONE;   // (the root is its own parent)
        depth[r] = 0;
        if (r == n_order) continue;
        const uint32_t c = node_scc[r];
        w[r] = c < n_scc && table[c].n_nodes == 1 ? SBW_REAL : 0u;
        cin[r] = cout[r] = total[r] = 0;
        exit_of[r] = encl[r] = CC_NONE;
        dead[r] = 0;
    }
}

__global__ __launch_bounds__(256) void k_sb_degrees(const EdgeRanks* __restrict__ er, uint32_t n_edges, uint32_t n_order,
                                                    const uint8_t* __restrict__ edge_class, uint32_t* __restrict__ w,
                                                    uint32_t* __restrict__ cin, uint32_t* __restrict__ cout,
                                                    unsigned long long* __restrict__ counters) {
    uint64_t c[1] = {0};
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        const EdgeRanks x = er[e];
        if (edge_class[e] != 1 || x.ru >= n_order || x.rv >= n_order) continue;
        if (x.ru == x.rv) {
            if (!(w[x.ru] & SBW_LOOP)) atomicOr(&w[x.ru], (uint32_t)SBW_LOOP);
            continue;
        }
        atomicAdd(&cout[x.ru], 1u);
        atomicAdd(&cin[x.rv], 1u);
        ++c[0];
    }
    block_add<1>(c, counters + BC_DEDGES);
}

__global__ __launch_bounds__(256) void k_sb_fill(const EdgeRanks* __restrict__ er, uint32_t n_edges, uint32_t n_order,
                                                 const uint8_t* __restrict__ edge_class, const uint32_t* __restrict__ cin,
                                                 const uint32_t* __restrict__ cout, const uint32_t* __restrict__ off_in,
                                                 const uint32_t* __restrict__ off_out, uint32_t* __restrict__ cur_in,
                                                 uint32_t* __restrict__ cur_out, uint32_t* __restrict__ list_in,
                                                 uint32_t* __restrict__ list_out) {
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        const EdgeRanks x = er[e];
        if (edge_class[e] != 1 || x.ru >= n_order || x.rv >= n_order || x.ru == x.rv) continue;
        const uint32_t i = atomicAdd(&cur_in[x.rv], 1u), o = atomicAdd(&cur_out[x.ru], 1u);
        const uint64_t at_in = (uint64_t)off_in[x.rv] + i, at_out = (uint64_t)off_out[x.ru] + o;
        if (i < cin[x.rv] && at_in < n_edges) list_in[at_in] = x.ru;       // (never index on trust)
        if (o < cout[x.ru] && at_out < n_edges) list_out[at_out] = x.rv;
    }
}

__global__ __launch_bounds__(256) void k_sb_nodes(uint32_t n_order, const uint8_t* __restrict__ flags, const uint32_t* __restrict__ cin,
                                                  const uint32_t* __restrict__ cout, uint32_t* __restrict__ w,
                                                  uint32_t* __restrict__ lvl_f, uint32_t* __restrict__ lvl_b,
                                                  unsigned long long* __restrict__ counters) {
    uint64_t c[3] = {0, 0, 0};   // self-loop ranks, ('r_', v) edges, (u, 're_') edges
    uint64_t real = 0;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        uint32_t x = w[r];
        const uint32_t f = flags[r];
        if (!(x & SBW_REAL)) {
            lvl_f[r] = lvl_b[r] = 0;
            continue;
        }
        if ((f & SF_R_IN) || cin[r] == 0) x |= SBW_SOURCE;
        if ((f & SF_RE_OUT) || cout[r] == 0) x |= SBW_SINK;
        w[r] = x;
        lvl_f[r] = lvl_b[r] = 1;
        ++real;
        c[0] += (x & SBW_LOOP) != 0;
        c[1] += (f & (SF_R_IN | SF_START)) != 0;
        c[2] += (f & (SF_RE_OUT | SF_SINK)) != 0;
    }
    block_add<3>(c, counters + BC_LOOPS);
    const uint64_t s = wave_sum64(real);
    if (lane_id() == 0 && s) atomicAdd(&counters[BC_REAL], (unsigned long long)s);
}
static_assert(BC_R_EDGES == BC_LOOPS + 1 && BC_RE_EDGES == BC_LOOPS + 2, "k_sb_nodes adds the three in one go");

__global__ __launch_bounds__(256) void k_sb_level(const EdgeRanks* __restrict__ er, uint32_t n_edges, uint32_t n_order,
                                                  const uint8_t* __restrict__ edge_class, uint32_t* __restrict__ lvl_f,
                                                  uint32_t* __restrict__ lvl_b, unsigned long long* __restrict__ changed) {
    uint64_t c[1] = {0};
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        const EdgeRanks x = er[e];
        if (edge_class[e] != 1 || x.ru >= n_order || x.rv >= n_order || x.ru == x.rv) continue;
        const uint32_t f = lvl_f[x.ru] + 1, b = lvl_b[x.rv] + 1;
        if (f > lvl_f[x.rv]) c[0] += atomicMax(&lvl_f[x.rv], f) < f;
        if (b > lvl_b[x.ru]) c[0] += atomicMax(&lvl_b[x.ru], b) < b;
    }
    const uint64_t s = wave_sum64(c[0]);
    if (lane_id() == 0 && s) atomicAdd(changed, (unsigned long long)s);
}

__global__ __launch_bounds__(256) void k_sb_level_max(uint32_t n_order, const uint32_t* __restrict__ lvl_f,
                                                      const uint32_t* __restrict__ lvl_b, unsigned long long* __restrict__ counters) {
    unsigned long long mf = 0, mb = 0;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        mf = lvl_f[r] > mf ? lvl_f[r] : mf;
        mb = lvl_b[r] > mb ? lvl_b[r] : mb;
    }
    if (mf) atomicMax(&counters[BC_LEVF], mf);
    if (mb) atomicMax(&counters[BC_LEVB], mb);
}

// one level of one tree: `lvl`, `off` / `deg` / `list` and `top` are the forward ones (levels from the sources, parents,
// SBW_SOURCE) for idom, the backward ones (levels from the sinks, children, SBW_SINK) for ipdom
__global__ __launch_bounds__(256) void k_sb_tree(uint32_t n_order, uint32_t n_edges, uint32_t level, const uint32_t* __restrict__ lvl,
                                                 const uint32_t* __restrict__ off, const uint32_t* __restrict__ deg,
                                                 const uint32_t* __restrict__ list, const uint32_t* __restrict__ w, uint32_t top,
                                                 uint32_t* idom, uint32_t* depth,   // (read on lower levels, written on this one)
                                                 unsigned long long* __restrict__ counters) {
    uint64_t bad = 0;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        if (lvl[r] != level) continue;
        uint32_t d = (w[r] & top) ? n_order : CC_NONE;
        const uint32_t first = off[r], k = deg[r];
        bool failed = (uint64_t)first + k > n_edges;
        for (uint32_t i = 0; i < k && !failed; ++i) {
            const uint32_t p = list[first + i];
            if (p >= n_order || lvl[p] >= level) failed = true;   // (a neighbour on the root's side lies on a lower level)
            else d = d == CC_NONE ? p : sb_lca(d, p, idom, depth, n_order, 2 * level + 2, failed);
        }
        if (failed || d == CC_NONE) {
            ++bad;
            continue;
        }
        idom[r] = d;
        depth[r] = depth[d] + 1;
    }
    const uint64_t s = wave_sum64(bad);
    if (lane_id() == 0 && s) atomicAdd(&counters[BC_WALK], (unsigned long long)s);
}

__global__ __launch_bounds__(256) void k_sb_pairs(uint32_t n_order, const uint32_t* __restrict__ w, const uint32_t* __restrict__ idom,
                                                  const uint32_t* __restrict__ ipdom, uint32_t* __restrict__ exit_of) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        if (!(w[r] & SBW_REAL)) continue;
        const uint32_t t = ipdom[r];
        if (t < n_order && idom[t] == r) exit_of[r] = t;
    }
}

__global__ __launch_bounds__(256) void k_sb_encl(uint32_t n_order, uint32_t level, const uint32_t* __restrict__ lvl_f,
                                                 const uint32_t* __restrict__ idom, const uint32_t* __restrict__ exit_of,
                                                 uint32_t* __restrict__ encl) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        if (lvl_f[r] != level) continue;
        const uint32_t d = idom[r];
        if (d >= n_order) continue;   // (the root, or a rank whose walk failed: no bubble holds it)
        const uint32_t t = exit_of[d];
        encl[r] = t != CC_NONE && t != r ? d : encl[d];
    }
}

__global__ __launch_bounds__(256) void k_sb_dead_init(uint32_t n_order, const uint32_t* __restrict__ w, const uint32_t* __restrict__ idom,
                                                      const uint32_t* __restrict__ exit_of, const uint32_t* __restrict__ encl,
                                                      uint8_t* __restrict__ dead) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        if (!(w[r] & SBW_LOOP) || !(w[r] & SBW_REAL)) continue;
        if (exit_of[r] != CC_NONE) dead[r] = 1;   // (every writer stores the same value)
        const uint32_t d = idom[r], x = encl[r];
        if (d < n_order && exit_of[d] == r) dead[d] = 1;
        if (x < n_order) dead[x] = 1;
    }
}

__global__ __launch_bounds__(256) void k_sb_dead_round(uint32_t n_order, const uint32_t* __restrict__ exit_of,
                                                       const uint32_t* __restrict__ encl, uint8_t* __restrict__ dead,
                                                       unsigned long long* __restrict__ changed) {
    uint64_t c[1] = {0};
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        if (exit_of[r] == CC_NONE || !dead[r]) continue;
        const uint32_t x = encl[r];
        if (x < n_order && !dead[x]) {
            dead[x] = 1;
            ++c[0];
        }
    }
    const uint64_t s = wave_sum64(c[0]);
    if (lane_id() == 0 && s) atomicAdd(changed, (unsigned long long)s);
}

__global__ __launch_bounds__(256) void k_sb_label(uint32_t n_order, const uint32_t* __restrict__ node_at, const uint32_t* __restrict__ w,
                                                  const uint32_t* __restrict__ idom, const uint32_t* __restrict__ exit_of,
                                                  const uint32_t* __restrict__ encl, const uint8_t* __restrict__ dead,
                                                  uint32_t* __restrict__ inside, uint32_t* __restrict__ total, uint8_t* __restrict__ root,
                                                  uint32_t* __restrict__ exit_out, uint32_t* __restrict__ inside_out,
                                                  uint8_t* __restrict__ flags_out, unsigned long long* __restrict__ counters) {
    uint64_t c[2] = {0, 0};   // nested, discarded
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        const uint32_t x = w[r], t = exit_of[r], d = idom[r], in = encl[r];
        uint32_t f = (x & SBW_REAL) && (x & SBW_LOOP) ? SB_SELF_LOOP : 0u;
        const bool enters = t < n_order && !dead[r];
        const uint32_t holder = in < n_order && !dead[in] ? in : CC_NONE;
        if (enters) f |= SB_ENTRANCE | (holder != CC_NONE ? SB_NESTED : 0u);
        if (d < n_order && exit_of[d] == r && !dead[d]) f |= SB_EXIT;
        c[0] += enters && holder != CC_NONE;
        c[1] += t < n_order && !enters;
        root[r] = enters;
        inside[r] = holder;
        if (holder != CC_NONE) atomicAdd(&total[holder], 1u);
        exit_out[r] = enters ? node_at[t] : CC_NONE;
        inside_out[r] = holder != CC_NONE ? node_at[holder] : CC_NONE;
        flags_out[r] = (uint8_t)f;
    }
    block_add<2>(c, counters + BC_NESTED);
}
static_assert(BC_DISCARDED == BC_NESTED + 1, "k_sb_label adds the two in one go");

__global__ __launch_bounds__(256) void k_sb_sum(uint32_t n_order, uint32_t level, const uint32_t* __restrict__ lvl_f,
                                                const uint8_t* __restrict__ root, const uint32_t* __restrict__ inside,
                                                uint32_t* __restrict__ total) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        if (lvl_f[r] != level || !root[r]) continue;
        const uint32_t x = inside[r];
        if (x < n_order) atomicAdd(&total[x], total[r]);   // (total[r] is final: what it holds lies on higher levels)
    }
}

__global__ __launch_bounds__(256) void k_sb_table(uint32_t n_order, uint32_t n_bubbles, const uint32_t* __restrict__ node_at,
                                                  const uint8_t* __restrict__ root, const uint32_t* __restrict__ index,
                                                  const uint32_t* __restrict__ exit_of, const uint32_t* __restrict__ inside,
                                                  const uint32_t* __restrict__ total, Bubble* __restrict__ table) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        if (!root[r]) continue;
        const uint32_t i = index[r], t = exit_of[r];
        if (i >= n_bubbles || t >= n_order) continue;   // (cannot happen: the prefix sum counted this rank)
        table[i] = Bubble{node_at[r], node_at[t], total[r], inside[r] < n_order ? 1u : 0u};
    }
}

}  // namespace po
