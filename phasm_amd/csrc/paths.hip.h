// Device side of what BubbleChainPhaser.phase() of `phasm phase` computes per bubble before it looks at a read (DESIGN.md
// section 3.9r):
//   networkx.all_simple_paths(g, entrance, exit)              phasm/phasing.py:196-234
//   superbubble_nodes(g, entrance, exit) - {entrance, exit}
//   the predecessors of the exit with their edge lengths      phasing.py:396 (_get_max_possible_overlap)
// on a graph result in HBM, behind the bubble-chain stage of bubblechains.hip.h (po_phase_paths runs it first with
// min_nodes = 1 and works on its words per rank: the top-level entrance bit, exit_of, `top` -- the outermost holder of a
// rank that lies strictly inside a bubble --, pred -- the top-level entrance whose bubble a rank exits --, n_inside, chain
// and position).
//
// The scheme works on RANKS.  A MEMBER of bubble (s, t) is s or a rank strictly inside, home[member] = s; t is no member
// (it may be the entrance of the next bubble: its count as an end is 1, whatever it counts as an entrance).  A rank is a
// member of at most one bubble, so the count and the done word of a member are indexed by rank.
//   k_pp_chain_counts                          bubbles per chain, for the prefix sum that numbers the bubbles by
//                                              (chain, position)
//   k_pp_bubbles                               per rank: home, the number of the bubble it enters, entrance per bubble
//   k_pp_keys                                  per edge: (tail rank << 32 | edge index) when the tail is a member, (head
//                                              rank << 32 | edge index) when the head exits a top-level bubble, else all
//                                              ones; an out-edge of a member that leaves U + {t} is a STRAY edge (counted;
//                                              the definition makes that 0).  Behind the bitonic sort of each array the
//                                              edges of one tail (head) stand together in edge order
//   k_pp_segments                              first and one-past-last place of every tail (head): a compare with the
//                                              neighbour
//   k_pp_count                                 one round: a member that is not done and whose successors inside the bubble
//                                              were all done by an EARLIER launch (done[w] holds the number of the launch
//                                              that wrote it; a word of this launch, or a stale 0, is "not yet") sums their
//                                              counts in successor order with a saturating add, stores the sum, then its
//                                              launch number.  A member is written by its own lane only: no atomics on the
//                                              counts, and the number of rounds is the same on every run
//   k_pp_table                                 per bubble: the table entry, its flags, the number of paths to list, of
//                                              predecessors and of interior nodes (three prefix sums follow)
//   k_pp_walk<false> / k_pp_walk<true>         ONE LANE PER LISTED PATH: lane (bubble, j) walks from s; at v it scans the
//                                              successors in order, subtracting counts until j < cnt[w], takes w, until t.
//                                              The first pass stores the length, the second -- behind the prefix sum of the
//                                              lengths -- the nodes.  Bounded by n_inside + 1 steps; a lane that gets there
//                                              without t, or finds no successor to take, raises a counter
//   k_pp_bubble_nodes                          n_path_nodes of every bubble from the two offset arrays
//   k_pp_preds                                 per sorted in-edge of an exit: (tail node, weight) at its bubble's offset
//   k_pp_inside_keys / k_pp_inside             (bubble << 32 | rank) of every rank strictly inside; behind the sort the
//                                              interior nodes of all bubbles back to back, ascending in rank
// No kernel follows links in an unbounded loop: the host bounds the rounds (round_phase of components.hip.h), the walk is
// bounded by the bubble's size.  Integers only: every output is the same on every run.
#pragma once

namespace po {

enum { QK_STRAY = 0, QK_BAD = 1, QK_MAXIN = 2, QK_BARE = 3, QK_UNLISTED = 4, QK_SATURATED = 5, QK_LISTED = 6, QK_MAXPATHS = 7, QK_WALK = 8,
       QK_MAXLEN = 9, QK_INSIDE = 10, QK_N = 11 };

enum : uint32_t { PPF_BARE = 1, PPF_UNLISTED = 2, PPF_SATURATED = 4 };   // (PO_PATHS_* of the header)
constexpr unsigned long long PP_MANY = ~0ull;                             // (PO_PATHS_MANY)
constexpr unsigned long long PP_NO_KEY = ~0ull;
constexpr uint32_t PP_LIST_CLAMP = 0x7FFFFFFFu;   // what a bubble adds to the listed sum at the most: the host refuses 2^30

struct BubblePaths {
    uint32_t entrance, exit, chain, position, n_inside, flags;
    unsigned long long n_paths, n_path_nodes;
};

__device__ inline unsigned long long pp_sat_add(unsigned long long a, unsigned long long b) {
    const unsigned long long s = a + b;
    return s < a ? PP_MANY : s;
}

// one compare-exchange step of a bitonic sort of n_pad = 2^p keys: partner distance j inside runs of k
__global__ __launch_bounds__(256) void k_pp_bitonic(unsigned long long* __restrict__ key, uint32_t n_pad, uint32_t j, uint32_t k) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_pad; i += gridDim.x * blockDim.x) {
        const uint32_t p = i ^ j;
        if (p <= i || p >= n_pad) continue;
        const unsigned long long a = key[i], b = key[p];
        const bool up = (i & k) == 0;
        if ((a > b) == up && a != b) {
            key[i] = b;
            key[p] = a;
        }
    }
}

__global__ __launch_bounds__(256) void k_pp_chain_counts(uint32_t n_chains, const BubbleChain* __restrict__ chains, uint32_t* __restrict__ nb) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= n_chains; i += gridDim.x * blockDim.x)
        nb[i] = i < n_chains ? chains[i].n_bubbles : 0u;
}

__global__ __launch_bounds__(256) void k_pp_bubbles(uint32_t n_order, uint32_t n_chains, uint32_t n_bubbles, const uint32_t* __restrict__ fw,
                                                    const uint32_t* __restrict__ top, const uint32_t* __restrict__ chain,
                                                    const uint32_t* __restrict__ pos, const uint32_t* __restrict__ coff,
                                                    const uint32_t* __restrict__ total, uint32_t* __restrict__ home,
                                                    uint32_t* __restrict__ bidx, uint32_t* __restrict__ bent, uint32_t* __restrict__ done,
                                                    unsigned long long* __restrict__ cnt, unsigned long long* __restrict__ counters) {
    uint64_t c[1] = {0};
    unsigned long long most = 0;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        const bool is_top = fw[r] & BCW_TOP;
        uint32_t hm = CC_NONE, b = CC_NONE;
        if (is_top) {
            const uint32_t ch = chain[r], p = pos[r];
            if (ch < n_chains && p < n_bubbles && coff[ch] + p < n_bubbles && coff[ch] + p < coff[ch + 1]) {
                hm = r;
                b = coff[ch] + p;
                bent[b] = r;   // (chain and position name one bubble: one writer)
                most = total[r] > most ? total[r] : most;
            } else {
                ++c[0];        // (cannot happen with min_nodes = 1: every top-level entrance lies in a reported chain)
            }
        } else {
            const uint32_t t = top[r];
            if (t < n_order) {
                if (fw[t] & BCW_TOP) hm = t;
                else ++c[0];   // (the outermost holder is no top-level entrance: an error on the host)
            }
        }
        home[r] = hm;
        bidx[r] = b;
        done[r] = 0;
        cnt[r] = 0;
    }
    most = merge_wave_max(most);
    if (lane_id() == 0 && most) atomicMax(&counters[QK_MAXIN], most);
    block_add<1>(c, counters + QK_BAD);
}

__global__ __launch_bounds__(256) void k_pp_keys(const EdgeRanks* __restrict__ er, uint32_t n_edges, uint32_t n_order, uint32_t n_pad,
                                                 const uint32_t* __restrict__ home, const uint32_t* __restrict__ exit_of,
                                                 const uint32_t* __restrict__ pred, unsigned long long* __restrict__ key_out,
                                                 unsigned long long* __restrict__ key_in, unsigned long long* __restrict__ counters) {
    uint64_t c[1] = {0};
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_pad; e += gridDim.x * blockDim.x) {
        unsigned long long ko = PP_NO_KEY, ki = PP_NO_KEY;
        if (e < n_edges) {
            const EdgeRanks x = er[e];
            if (x.ru < n_order && x.rv < n_order) {
                const uint32_t hm = home[x.ru];
                if (hm < n_order) {
                    ko = ((unsigned long long)x.ru << 32) | e;
                    if (x.rv != exit_of[hm] && (home[x.rv] != hm || x.rv == hm)) ++c[0];
                }
                if (pred[x.rv] < n_order) ki = ((unsigned long long)x.rv << 32) | e;
            }
        }
        key_out[e] = ko;
        key_in[e] = ki;
    }
    block_add<1>(c, counters + QK_STRAY);
}

// (first and last are cleared by the host: a rank without an edge of the kind keeps the empty range [0, 0))
__global__ __launch_bounds__(256) void k_pp_segments(const unsigned long long* __restrict__ key, uint32_t n_edges, uint32_t n_order,
                                                     uint32_t* __restrict__ first, uint32_t* __restrict__ last) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_edges; i += gridDim.x * blockDim.x) {
        const unsigned long long k = key[i];
        if (k == PP_NO_KEY) continue;
        const uint32_t r = (uint32_t)(k >> 32);
        if (r >= n_order) continue;
        if (i == 0 || (uint32_t)(key[i - 1] >> 32) != r) first[r] = i;
        if (i + 1 == n_edges || (uint32_t)(key[i + 1] >> 32) != r) last[r] = i + 1;
    }
}

// the count of successor w of a member of the bubble (hm, t): 1 at the exit, the member's own inside, 0 on a stray edge
__device__ inline bool pp_inside(uint32_t w, uint32_t hm, uint32_t n_order, const uint32_t* __restrict__ home) {
    return w < n_order && w != hm && home[w] == hm;
}

__global__ __launch_bounds__(256) void k_pp_count(uint32_t n_order, uint32_t n_edges, uint32_t launch, const uint32_t* __restrict__ home,
                                                  const uint32_t* __restrict__ exit_of, const uint32_t* __restrict__ first,
                                                  const uint32_t* __restrict__ last, const unsigned long long* __restrict__ key,
                                                  const EdgeRanks* __restrict__ er, uint32_t* done, unsigned long long* cnt,
                                                  unsigned long long* __restrict__ changed) {
    uint64_t c[1] = {0};
    for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n_order; v += gridDim.x * blockDim.x) {
        const uint32_t hm = home[v];
        if (hm >= n_order || done[v]) continue;
        const uint32_t t = exit_of[hm], i1 = last[v] <= n_edges ? last[v] : n_edges;
        unsigned long long sum = 0;
        bool ready = true;
        for (uint32_t i = first[v]; i < i1; ++i) {
            const uint32_t e = (uint32_t)key[i];
            if (e >= n_edges) continue;
            const uint32_t w = er[e].rv;
            if (w == t) {
                sum = pp_sat_add(sum, 1ull);
            } else if (pp_inside(w, hm, n_order, home)) {
                const uint32_t d = done[w];
                if (d == 0 || d >= launch) {
                    ready = false;
                    break;
                }
                sum = pp_sat_add(sum, cnt[w]);
            }
        }
        if (!ready) continue;
        cnt[v] = sum;
        done[v] = launch;
        ++c[0];
    }
    const uint64_t s = wave_sum64(c[0]);
    if (lane_id() == 0 && s) atomicAdd(changed, (unsigned long long)s);
}

__global__ __launch_bounds__(256) void k_pp_table(uint32_t n_bubbles, uint32_t n_order, unsigned long long max_paths,
                                                  const uint32_t* __restrict__ bent, const uint32_t* __restrict__ exit_of,
                                                  const uint32_t* __restrict__ node_at, const uint32_t* __restrict__ chain,
                                                  const uint32_t* __restrict__ pos, const uint32_t* __restrict__ total,
                                                  const unsigned long long* __restrict__ cnt, const uint32_t* __restrict__ in_first,
                                                  const uint32_t* __restrict__ in_last, BubblePaths* __restrict__ table,
                                                  uint32_t* __restrict__ n_list, uint32_t* __restrict__ n_pred, uint32_t* __restrict__ n_in,
                                                  unsigned long long* __restrict__ counters) {
    uint64_t c[4] = {0, 0, 0, 0};   // bare, unlisted, saturated, paths to list
    unsigned long long most = 0;
    for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b <= n_bubbles; b += gridDim.x * blockDim.x) {
        if (b == n_bubbles) {   // (the closing entries of the three prefix sums)
            n_list[b] = n_pred[b] = n_in[b] = 0;
            continue;
        }
        const uint32_t s = bent[b];
        const uint32_t t = s < n_order ? exit_of[s] : CC_NONE;
        if (s >= n_order || t >= n_order) {   // (cannot happen: every bubble number has its entrance)
            table[b] = BubblePaths{CC_NONE, CC_NONE, CC_NONE, CC_NONE, 0, PPF_UNLISTED, 0, 0};
            n_list[b] = n_pred[b] = n_in[b] = 0;
            ++c[1];
            continue;
        }
        const unsigned long long np = cnt[s];
        const bool sat = np == PP_MANY, unlisted = sat || np > max_paths;
        const uint32_t inside = total[s], flags = (inside == 0 ? PPF_BARE : 0u) | (unlisted ? PPF_UNLISTED : 0u) | (sat ? PPF_SATURATED : 0u);
        table[b] = BubblePaths{node_at[s], node_at[t], chain[s], pos[s], inside, flags, np, 0};
        const uint32_t listed = unlisted ? 0u : (np > PP_LIST_CLAMP ? PP_LIST_CLAMP : (uint32_t)np);
        n_list[b] = listed;
        n_pred[b] = in_last[t] - in_first[t];
        n_in[b] = inside;
        most = np > most ? np : most;
        c[0] += inside == 0;
        c[1] += unlisted;
        c[2] += sat;
        c[3] += listed;
    }
    most = merge_wave_max(most);
    if (lane_id() == 0 && most) atomicMax(&counters[QK_MAXPATHS], most);
    block_add<4>(c, counters + QK_BARE);
}
static_assert(QK_UNLISTED == QK_BARE + 1 && QK_SATURATED == QK_BARE + 2 && QK_LISTED == QK_BARE + 3, "k_pp_table adds the four in one go");

// the last bubble b with off[b] <= p: off ascends over n + 1 entries, off[0] = 0, off[n] > p (bubbles that list nothing
// repeat the offset of the next one that does, so the last such entry is the bubble that holds path p)
__device__ inline uint32_t pp_bubble_of(const uint32_t* off, uint32_t n, uint32_t p) {
    uint32_t lo = 0, hi = n;   // (off[lo] <= p < off[hi])
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}

// One lane per listed path.  Lanes of neighbouring j share the front of their walk (lexicographic order), so a wave
// mostly takes the same branches early and diverges toward the end; a lane writes its own row of path_nodes front to back.
template <bool WRITE>
__global__ __launch_bounds__(256) void k_pp_walk(uint32_t n_listed, uint32_t n_bubbles, uint32_t n_order, uint32_t n_edges,
                                                 uint32_t n_path_nodes, const uint32_t* __restrict__ bpo, const uint32_t* __restrict__ bent,
                                                 const uint32_t* __restrict__ exit_of, const uint32_t* __restrict__ total,
                                                 const uint32_t* __restrict__ home, const uint32_t* __restrict__ first,
                                                 const uint32_t* __restrict__ last, const unsigned long long* __restrict__ key,
                                                 const EdgeRanks* __restrict__ er, const unsigned long long* __restrict__ cnt,
                                                 const uint32_t* __restrict__ node_at, uint32_t* __restrict__ plen,
                                                 const uint32_t* __restrict__ poff, uint32_t* __restrict__ path_nodes,
                                                 unsigned long long* __restrict__ counters) {
    uint64_t c[1] = {0};
    unsigned long long longest = 0;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p <= n_listed; p += gridDim.x * blockDim.x) {
        if (p == n_listed) {   // (the closing entry of the prefix sum of the lengths)
            if (!WRITE) plen[p] = 0;
            continue;
        }
        const uint32_t b = pp_bubble_of(bpo, n_bubbles, p);
        const uint32_t s = bent[b];
        uint32_t len = 1;
        bool ok = s < n_order;
        const uint32_t o0 = WRITE ? poff[p] : 0u, room = WRITE ? poff[p + 1] - o0 : 0u;
        if (ok) {
            const uint32_t t = exit_of[s], steps = total[s] + 1;
            unsigned long long j = p - bpo[b];
            uint32_t v = s;
            if (WRITE && room && o0 < n_path_nodes) path_nodes[o0] = node_at[s];
            ok = false;
            for (uint32_t step = 0; step < steps; ++step) {
                const uint32_t i1 = last[v] <= n_edges ? last[v] : n_edges;
                uint32_t w = CC_NONE;
                for (uint32_t i = first[v]; i < i1; ++i) {
                    const uint32_t e = (uint32_t)key[i];
                    if (e >= n_edges) continue;
                    const uint32_t x = er[e].rv;
                    const unsigned long long cw = x == t ? 1ull : (pp_inside(x, s, n_order, home) ? cnt[x] : 0ull);
                    if (j < cw) {
                        w = x;
                        break;
                    }
                    j -= cw;
                }
                if (w >= n_order) break;   // (no successor holds path j: the counts do not add up)
                if (WRITE && len < room && (uint64_t)o0 + len < n_path_nodes) path_nodes[o0 + len] = node_at[w];
                ++len;
                if (w == t) {
                    ok = true;
                    break;
                }
                v = w;
            }
        }
        if (!ok || (WRITE && len != room)) ++c[0];
        if (!WRITE) plen[p] = ok ? len : 0u;
        longest = len > longest ? len : longest;
    }
    if (!WRITE) {
        longest = merge_wave_max(longest);
        if (lane_id() == 0 && longest) atomicMax(&counters[QK_MAXLEN], longest);
    }
    block_add<1>(c, counters + QK_WALK);
}

__global__ __launch_bounds__(256) void k_pp_bubble_nodes(uint32_t n_bubbles, const uint32_t* __restrict__ bpo, const uint32_t* __restrict__ poff,
                                                         BubblePaths* __restrict__ table) {
    for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < n_bubbles; b += gridDim.x * blockDim.x)
        table[b].n_path_nodes = poff[bpo[b + 1]] - poff[bpo[b]];
}

__global__ __launch_bounds__(256) void k_pp_preds(uint32_t n_edges, uint32_t n_order, uint32_t n_preds, const unsigned long long* __restrict__ key,
                                                  const EdgeRanks* __restrict__ er, const Edge* __restrict__ edges,
                                                  const uint32_t* __restrict__ pred, const uint32_t* __restrict__ bidx,
                                                  const uint32_t* __restrict__ in_first, const uint32_t* __restrict__ pred_off,
                                                  const uint32_t* __restrict__ node_at, uint32_t* __restrict__ pred_node,
                                                  int32_t* __restrict__ pred_weight, unsigned long long* __restrict__ counters) {
    uint64_t c[1] = {0};
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_edges; i += gridDim.x * blockDim.x) {
        const unsigned long long k = key[i];
        if (k == PP_NO_KEY) continue;
        const uint32_t t = (uint32_t)(k >> 32), e = (uint32_t)k;
        const uint32_t s = t < n_order ? pred[t] : CC_NONE;
        const uint32_t b = s < n_order ? bidx[s] : CC_NONE;
        if (e >= n_edges || b == CC_NONE || i < in_first[t]) {
            ++c[0];
            continue;
        }
        const uint64_t o = (uint64_t)pred_off[b] + (i - in_first[t]);
        if (o >= n_preds || er[e].ru >= n_order) {
            ++c[0];
            continue;
        }
        pred_node[o] = node_at[er[e].ru];
        pred_weight[o] = edges[e].weight;
    }
    block_add<1>(c, counters + QK_BAD);
}

__global__ __launch_bounds__(256) void k_pp_inside_keys(uint32_t n_order, uint32_t n_pad, const uint32_t* __restrict__ home,
                                                        const uint32_t* __restrict__ bidx, unsigned long long* __restrict__ key,
                                                        unsigned long long* __restrict__ counters) {
    uint64_t c[1] = {0};
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_pad; r += gridDim.x * blockDim.x) {
        unsigned long long k = PP_NO_KEY;
        if (r < n_order) {
            const uint32_t hm = home[r];
            if (hm < n_order && hm != r && bidx[hm] != CC_NONE) {
                k = ((unsigned long long)bidx[hm] << 32) | r;
                ++c[0];
            }
        }
        key[r] = k;
    }
    block_add<1>(c, counters + QK_INSIDE);
}

__global__ __launch_bounds__(256) void k_pp_inside(uint32_t n_inside, uint32_t n_order, const unsigned long long* __restrict__ key,
                                                   const uint32_t* __restrict__ node_at, uint32_t* __restrict__ inside_nodes) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_inside; i += gridDim.x * blockDim.x) {
        const uint32_t r = (uint32_t)key[i];
        inside_nodes[i] = r < n_order ? node_at[r] : CC_NONE;
    }
}

}  // namespace po
