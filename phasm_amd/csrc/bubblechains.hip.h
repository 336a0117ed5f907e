// Device side of the bubble chains of `phasm chain`:
//   build_bubblechains(component, min_nodes)                  phasm/assembly_graph.py:594-652, called from cli/assembler.py:272
// on a graph result in HBM, behind the superbubble stage of superbubbles.hip.h (po_layout_bubblechains runs it first and
// works on its words per rank: the byte "enters a surviving bubble", exit_of, and `inside`, the entrance of the innermost
// surviving bubble that holds the rank strictly).
//
// The scheme works on RANKS.  A TOP-LEVEL entrance enters a surviving bubble and lies inside none.  Bubble (s, t) links to
// bubble (t, w) when both are top-level; a chain is a maximal run of links, its HEAD the entrance that no top-level bubble
// exits.  A node enters at most one bubble and exits at most one, so every scatter below has one writer per word.
//   k_bc_init                                  per rank: top-level entrance bit, top[r] = inside[r], the sums cleared
//   k_bc_link                                  per top-level entrance s with exit t: pred[t] = s (unique); next[s] = t iff t
//                                              is a top-level entrance itself
//   k_bc_heads                                 head bit (a top-level entrance without pred), last-exit bit (pred, but no
//                                              top-level entrance); the ranking's start: (jb, hops) = (pred, 1), a head and
//                                              every other rank (itself, 0)
//   k_bc_nest                                  pointer jumping along `top` to the entrance that is itself inside nothing:
//                                              top[v] = top[top[v]] while that exists.  IN PLACE: a word read as another
//                                              thread of the same launch left it is still an ancestor of v on the same
//                                              chain of holders, so a round only gets further with it; the round that ends
//                                              the loop wrote nothing
//   k_bc_jump                                  list ranking of the top-level entrances toward their head, as k_merge_jump
//                                              of merge.hip.h: hops += hops[jb]; jb = jb[jb] from one buffer pair into the
//                                              other (summing in place would add a hop count that the same launch has
//                                              already doubled).  A round counts the ranks whose jb moved; after k rounds a
//                                              rank d links behind its head holds min(d, 2^k) hops
//   k_bc_place                                 head and position of every rank: an entrance at its own, a last exit at those
//                                              of the bubble it exits, an inside rank at those of its outermost holder; +1
//                                              node (and +1 bubble for an entrance) at the head; the chain's one entrance
//                                              without next stores the last exit there
//   k_bc_edges                                 per edge with both ends under the same head: +1 edge at the head
//   k_bc_filter                                a head with at least min_nodes nodes survives: its byte for the scaffold's
//                                              prefix sum, the sums over the survivors
//   k_bc_table / k_bc_nodes / k_bc_edge_out    behind the prefix sum: the table in head-rank order, chain and position per
//                                              node, chain per edge
// No kernel follows links in a loop: the host bounds the rounds (round_phase of components.hip.h).  Integer atomics only:
// every output is the same on every run.
#pragma once

namespace po {

enum { HK_TOP = 0, HK_HEADS = 1, HK_BAD = 2, HK_SHORT = 3, HK_CHAINS = 4, HK_CNODES = 5, HK_CEDGES = 6, HK_MAXB = 7, HK_N = 8 };

enum : uint32_t { BCW_TOP = 1, BCW_HEAD = 2, BCW_LAST = 4 };

struct BubbleChain {
    uint32_t first_entrance, last_exit, n_bubbles, n_nodes;
    unsigned long long n_edges;
};

__global__ __launch_bounds__(256) void k_bc_init(uint32_t n_order, const uint8_t* __restrict__ enters, const uint32_t* __restrict__ inside,
                                                 uint32_t* __restrict__ fw, uint32_t* __restrict__ next, uint32_t* __restrict__ pred,
                                                 uint32_t* __restrict__ top, uint32_t* __restrict__ cb, uint32_t* __restrict__ cn,
                                                 unsigned long long* __restrict__ ce, uint32_t* __restrict__ last) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        const uint32_t in = inside[r];
        fw[r] = enters[r] && in >= n_order ? (uint32_t)BCW_TOP : 0u;
        top[r] = in < n_order ? in : CC_NONE;
        next[r] = pred[r] = last[r] = CC_NONE;
        cb[r] = cn[r] = 0;
        ce[r] = 0;
    }
}

__global__ __launch_bounds__(256) void k_bc_link(uint32_t n_order, const uint32_t* __restrict__ fw, const uint32_t* __restrict__ exit_of,
                                                 uint32_t* __restrict__ next, uint32_t* __restrict__ pred,
                                                 unsigned long long* __restrict__ counters) {
    uint64_t c[1] = {0};
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        if (!(fw[r] & BCW_TOP)) continue;
        ++c[0];
        const uint32_t t = exit_of[r];
        if (t >= n_order) continue;   // (cannot happen: the byte says the rank enters a bubble)
        pred[t] = r;                  // (a rank exits at most one bubble: one writer)
        if (fw[t] & BCW_TOP) next[r] = t;
    }
    block_add<1>(c, counters + HK_TOP);
}

__global__ __launch_bounds__(256) void k_bc_heads(uint32_t n_order, const uint32_t* __restrict__ pred, uint32_t* __restrict__ fw,
                                                  uint32_t* __restrict__ jb, uint32_t* __restrict__ hops,
                                                  unsigned long long* __restrict__ counters) {
    uint64_t c[1] = {0};
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        const uint32_t x = fw[r], p = pred[r];
        const bool top = x & BCW_TOP, linked = top && p < n_order;
        if (top && !linked) {
            fw[r] = x | BCW_HEAD;
            ++c[0];
        } else if (!top && p < n_order) {
            fw[r] = x | BCW_LAST;
        }
        jb[r] = linked ? p : r;
        hops[r] = linked ? 1u : 0u;
    }
    block_add<1>(c, counters + HK_HEADS);
}

__global__ __launch_bounds__(256) void k_bc_nest(uint32_t n_order, uint32_t* top, unsigned long long* __restrict__ changed) {
    uint64_t c[1] = {0};
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        const uint32_t a = top[r];
        if (a >= n_order) continue;
        const uint32_t b = top[a];
        if (b >= n_order) continue;   // (a is inside nothing: the outermost holder)
        top[r] = b;
        ++c[0];
    }
    const uint64_t s = wave_sum64(c[0]);
    if (lane_id() == 0 && s) atomicAdd(changed, (unsigned long long)s);
}

__global__ __launch_bounds__(256) void k_bc_jump(uint32_t n_order, const uint32_t* __restrict__ jb_in, const uint32_t* __restrict__ hops_in,
                                                 uint32_t* __restrict__ jb_out, uint32_t* __restrict__ hops_out,
                                                 unsigned long long* __restrict__ changed) {
    uint64_t c[1] = {0};
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        const uint32_t j = jb_in[r];
        if (j >= n_order) {   // (cannot happen: jb starts in range and only takes values of jb)
            jb_out[r] = r;
            hops_out[r] = 0;
            continue;
        }
        const uint32_t jj = jb_in[j];
        jb_out[r] = jj;
        hops_out[r] = hops_in[r] + hops_in[j];
        c[0] += jj != j;
    }
    const uint64_t s = wave_sum64(c[0]);
    if (lane_id() == 0 && s) atomicAdd(changed, (unsigned long long)s);
}

__global__ __launch_bounds__(256) void k_bc_place(uint32_t n_order, const uint32_t* __restrict__ fw, const uint32_t* __restrict__ next,
                                                  const uint32_t* __restrict__ pred, const uint32_t* __restrict__ top,
                                                  const uint32_t* __restrict__ exit_of, const uint32_t* __restrict__ jb,
                                                  const uint32_t* __restrict__ hops, uint32_t* __restrict__ nhead,
                                                  uint32_t* __restrict__ npos, uint32_t* __restrict__ cb, uint32_t* __restrict__ cn,
                                                  uint32_t* __restrict__ last, unsigned long long* __restrict__ counters) {
    uint64_t c[1] = {0};
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        const uint32_t x = fw[r];
        const uint32_t s = (x & BCW_TOP) ? r : (x & BCW_LAST) ? pred[r] : top[r];   // the entrance whose bubble holds r
        uint32_t head = CC_NONE, pos = CC_NONE;
        if (s < n_order) {
            const uint32_t hd = jb[s];
            if (!(fw[s] & BCW_TOP) || hd >= n_order || !(fw[hd] & BCW_HEAD)) {
                ++c[0];   // (the holder is no top-level entrance or its ranking reached no head: an error on the host)
            } else {
                head = hd;
                pos = hops[s];
                atomicAdd(&cn[head], 1u);
                if (x & BCW_TOP) {
                    atomicAdd(&cb[head], 1u);
                    if (next[r] >= n_order) last[head] = exit_of[r];   // (the chain's one entrance without a link out)
                }
            }
        }
        nhead[r] = head;
        npos[r] = pos;
    }
    block_add<1>(c, counters + HK_BAD);
}

__global__ __launch_bounds__(256) void k_bc_edges(const EdgeRanks* __restrict__ er, uint32_t n_edges, uint32_t n_order,
                                                  const uint32_t* __restrict__ nhead, unsigned long long* __restrict__ ce) {
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        const EdgeRanks x = er[e];
        if (x.ru >= n_order || x.rv >= n_order) continue;
        const uint32_t hd = nhead[x.ru];
        if (hd < n_order && hd == nhead[x.rv]) atomicAdd(&ce[hd], 1ull);
    }
}

__global__ __launch_bounds__(256) void k_bc_filter(uint32_t n_order, uint32_t min_nodes, const uint32_t* __restrict__ fw,
                                                   const uint32_t* __restrict__ cb, const uint32_t* __restrict__ cn,
                                                   const unsigned long long* __restrict__ ce, uint8_t* __restrict__ root,
                                                   unsigned long long* __restrict__ counters) {
    uint64_t c[4] = {0, 0, 0, 0};   // short, chains, their nodes, their edges
    unsigned long long mb = 0;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        const bool head = fw[r] & BCW_HEAD, keep = head && cn[r] >= min_nodes;
        root[r] = keep;
        if (!head) continue;
        mb = cb[r] > mb ? cb[r] : mb;
        c[0] += !keep;
        c[1] += keep;
        c[2] += keep ? cn[r] : 0u;
        c[3] += keep ? ce[r] : 0ull;
    }
    block_add<4>(c, counters + HK_SHORT);
    if (mb) atomicMax(&counters[HK_MAXB], mb);
}
static_assert(HK_CHAINS == HK_SHORT + 1 && HK_CNODES == HK_SHORT + 2 && HK_CEDGES == HK_SHORT + 3, "k_bc_filter adds the four in one go");

__global__ __launch_bounds__(256) void k_bc_table(uint32_t n_order, uint32_t n_chains, const uint32_t* __restrict__ node_at,
                                                  const uint8_t* __restrict__ root, const uint32_t* __restrict__ index,
                                                  const uint32_t* __restrict__ last, const uint32_t* __restrict__ cb,
                                                  const uint32_t* __restrict__ cn, const unsigned long long* __restrict__ ce,
                                                  BubbleChain* __restrict__ table) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        if (!root[r]) continue;
        const uint32_t i = index[r], t = last[r];
        if (i >= n_chains) continue;   // (cannot happen: the prefix sum counted this rank)
        table[i] = BubbleChain{node_at[r], t < n_order ? node_at[t] : CC_NONE, cb[r], cn[r], ce[r]};
    }
}

__global__ __launch_bounds__(256) void k_bc_nodes(uint32_t n_order, uint32_t n_chains, const uint8_t* __restrict__ root,
                                                  const uint32_t* __restrict__ index, const uint32_t* __restrict__ nhead,
                                                  const uint32_t* __restrict__ npos, uint32_t* __restrict__ chain_out,
                                                  uint32_t* __restrict__ bubble_out) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        const uint32_t hd = nhead[r];
        const bool kept = hd < n_order && root[hd] && index[hd] < n_chains;
        chain_out[r] = kept ? index[hd] : CC_NONE;
        bubble_out[r] = kept ? npos[r] : CC_NONE;
    }
}

__global__ __launch_bounds__(256) void k_bc_edge_out(const EdgeRanks* __restrict__ er, uint32_t n_edges, uint32_t n_order,
                                                     const uint32_t* __restrict__ chain_of, uint32_t* __restrict__ edge_out) {
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        const EdgeRanks x = er[e];
        uint32_t c = CC_NONE;
        if (x.ru < n_order && x.rv < n_order && chain_of[x.ru] == chain_of[x.rv]) c = chain_of[x.ru];
        edge_out[e] = c;
    }
}

}  // namespace po
