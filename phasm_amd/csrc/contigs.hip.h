// Device side of the contigs of `phasm chain`:
//   identify_contigs(component, bubblechain_nodes, min_length)  phasm/assembly_graph.py:655-718, called from cli/assembler.py:289
// on a graph result in HBM, behind the rank scaffold (components.hip.h) and, when the caller gives no exclude set, behind
// the bubble-chain stage of bubblechains.hip.h (the chain word per rank says which ranks are excluded).
//
// The scheme works on EDGES, in the graph's edge order.  With in / out the degrees of a rank, edge (a, b) is a ROOT START when
// in(a) != 1, a LATE START when in(a) == 1 and out(a) > 1, an EXTENSION when in(a) == 1 and out(a) == 1; a start with both
// ends excluded is BLOCKED.  An extension belongs to the path of the one in-edge of a; a late start is covered iff the head
// of the path of that in-edge is and it is not blocked.  Both are list rankings toward a root, on edges.
//   k_ct_init                                  per rank: degrees cleared, the one in-edge unknown, the length of
//                                              the node (a read's from the handle, a merged node's from the result), the
//                                              exclude byte (the caller's, or "carries a chain")
//   k_ct_degrees                               per edge: +1 out at rank u, +1 in at rank v, ine[v] = the edge (one writer per
//                                              word wherever the in-degree is 1, and only there the word is read)
//   k_ct_classes                               per edge: the class byte and the blocked bit
//   k_ct_links                                 the ranking's start: a start (itself, 0 hops, weight sum 0); an extension (the
//                                              in-edge of its first node, 1 hop, its own weight).  Bit 31 of the link word
//                                              says that the edge it names is a start: the entry is RESOLVED
//   k_ct_jump                                  hops += hops[jb]; sum += sum[jb]; jb = jb[jb], from one buffer triple into the
//                                              other (as k_bc_jump, and for its reason).  A resolved entry is copied.  The
//                                              round counts the entries it RESOLVED: entries on rings of in-degree-1 nodes
//                                              never reach a start, so "nothing moved" never comes.  After k rounds an entry d
//                                              edges behind its head is resolved iff d <= 2^k, and the depths are downward
//                                              closed, so the first round that resolves nothing is the last
//   k_ct_cover_init                            per start: a root start is FINAL (link = itself, bit 31; ok = not blocked); a
//                                              late start whose in-edge reached no head is DEAD, final too (ok = 0); every
//                                              other late start links to the head of the path that ends at its first node,
//                                              bit 31 set and that head's ok ANDed in iff the head is final
//   k_ct_cover_jump                            ok &= ok[cj]; cj = cj[cj], between two buffer pairs, counting the resolved
//   k_ct_paths                                 per edge: covered iff its head's link is final and its ok is 1; the LAST edge
//                                              of a path (its second node does not have in == out == 1) stores the node
//                                              count, weight sum + length of the last node, and the last rank at the head:
//                                              one writer per head
//   k_ct_filter / k_ct_isolated                a covered head with length >= min_contig_len survives (its byte for the prefix
//                                              sum over the edges); a rank with in == out == 0 and a long enough node too (its
//                                              byte for the scaffold's prefix sum over the ranks); the sums
//   k_ct_keys / k_merge_bitonic / k_ct_number  the surviving heads sorted by (rank of the first node, edge index): contig
//                                              j of the head, its table entry
//   k_ct_iso_table / k_ct_edge_out             the one-node contigs behind them by rank; contig and place per edge
// No kernel walks a path in a loop: the host bounds the rounds (round_phase of components.hip.h).  Weight sums are formed in
// unsigned 64-bit arithmetic (an entry on a ring doubles its sum every round until the loop ends; it is never read) and read
// as signed.  Integer atomics only: every output is the same on every run.
// Memory beyond the rank scaffold, all of it allocated before the first launch: 49 bytes per node (25 of words and bytes, 24
// of table room) and at most 120 per edge (72 of words and bytes, 24 of table room, 12 per place of the sort, which pads
// edges + 1 to a power of two: below 24).  Without an exclude set from the caller the three stages of
// po_layout_bubblechains come first, in their own workspaces (260 per node, 21 per edge): 309 per node and 141 per edge.
#pragma once

namespace po {

enum { TK_EXCLUDED = 0, TK_ROOT = 1, TK_LATE = 2, TK_BLOCKED = 3, TK_COVERED = 4, TK_UNCOVERED = 5, TK_PATHS = 6, TK_SHORT = 7, TK_KEPT = 8,
       TK_PEDGES = 9, TK_ISO = 10, TK_SHORTISO = 11, TK_MAXN = 12, TK_BAD = 13, TK_N = 14 };

enum : uint8_t { CTC_START = 1, CTC_LATE = 2, CTC_BLOCKED = 4 };   // (an extension is 0; a late start START | LATE)
constexpr uint32_t CT_DONE = 0x80000000u;                           // bit 31 of a link word: the edge it names is a root of the ranking

struct Contig {
    uint32_t first_node, last_node, n_nodes, first_edge;
    long long length;
};

__device__ inline bool ct_long_enough(long long length, unsigned long long min_len) {
    return length >= 0 && (unsigned long long)length >= min_len;
}

__global__ __launch_bounds__(256) void k_ct_init(uint32_t n_order, const uint32_t* __restrict__ node_at, uint32_t n_ids, uint32_t n_total,
                                                 const uint32_t* __restrict__ len, const long long* __restrict__ mlen,
                                                 const uint32_t* __restrict__ chain_of, uint8_t* __restrict__ excl,
                                                 uint32_t* __restrict__ indeg, uint32_t* __restrict__ outdeg, uint32_t* __restrict__ ine,
                                                 long long* __restrict__ nlen,
                                                 unsigned long long* __restrict__ counters) {
    uint64_t c[1] = {0};
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        indeg[r] = outdeg[r] = 0;
        ine[r] = CC_NONE;
        const uint32_t id = node_at[r];
        nlen[r] = id < n_ids ? (long long)len[id] : (id < n_total && mlen) ? mlen[id - n_ids] : 0ll;
        if (chain_of) excl[r] = chain_of[r] != CC_NONE;
        c[0] += excl[r] != 0;
    }
    block_add<1>(c, counters + TK_EXCLUDED);
}

__global__ __launch_bounds__(256) void k_ct_degrees(const EdgeRanks* __restrict__ er, uint32_t n_edges, uint32_t n_order,
                                                    uint32_t* __restrict__ indeg, uint32_t* __restrict__ outdeg, uint32_t* __restrict__ ine) {
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        const EdgeRanks x = er[e];
        if (x.ru >= n_order || x.rv >= n_order) continue;
        atomicAdd(&outdeg[x.ru], 1u);
        atomicAdd(&indeg[x.rv], 1u);
        ine[x.rv] = e;   // (read only where the in-degree is 1: one writer)
    }
}

__global__ __launch_bounds__(256) void k_ct_classes(const EdgeRanks* __restrict__ er, uint32_t n_edges, uint32_t n_order,
                                                    const uint32_t* __restrict__ indeg, const uint32_t* __restrict__ outdeg,
                                                    const uint8_t* __restrict__ excl, uint8_t* __restrict__ cls,
                                                    unsigned long long* __restrict__ counters) {
    uint64_t c[3] = {0, 0, 0};   // root starts, late starts, blocked starts
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        const EdgeRanks x = er[e];
        uint8_t k = 0;
        if (x.ru < n_order && x.rv < n_order) {
            const uint32_t in = indeg[x.ru], out = outdeg[x.ru];
            if (in != 1) k = CTC_START;
            else if (out > 1) k = CTC_START | CTC_LATE;
            if (k && excl[x.ru] && excl[x.rv]) k |= CTC_BLOCKED;
            c[0] += k && !(k & CTC_LATE);
            c[1] += (k & CTC_LATE) != 0;
            c[2] += (k & CTC_BLOCKED) != 0;
        }
        cls[e] = k;
    }
    block_add<3>(c, counters + TK_ROOT);
}
static_assert(TK_LATE == TK_ROOT + 1 && TK_BLOCKED == TK_ROOT + 2, "k_ct_classes adds the three in one go");

__global__ __launch_bounds__(256) void k_ct_links(const EdgeRanks* __restrict__ er, const Edge* __restrict__ edges, uint32_t n_edges,
                                                  uint32_t n_order, const uint32_t* __restrict__ ine, const uint8_t* __restrict__ cls,
                                                  uint32_t* __restrict__ jb, uint32_t* __restrict__ hops,
                                                  unsigned long long* __restrict__ ws) {
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        const uint32_t ru = er[e].ru;
        const uint32_t p = (cls[e] & CTC_START) || ru >= n_order ? e : ine[ru];
        if (p == e || p >= n_edges) {   // a start; an extension that is its own in-edge (a self-loop) resolves never
            const bool start = cls[e] & CTC_START;
            jb[e] = start ? (e | CT_DONE) : e;
            hops[e] = start ? 0u : 1u;
            ws[e] = start ? 0ull : (unsigned long long)(long long)edges[e].weight;
            continue;
        }
        jb[e] = (cls[p] & CTC_START) ? (p | CT_DONE) : p;
        hops[e] = 1;
        ws[e] = (unsigned long long)(long long)edges[e].weight;
    }
}

__global__ __launch_bounds__(256) void k_ct_jump(uint32_t n_edges, const uint32_t* __restrict__ jb_in, const uint32_t* __restrict__ hops_in,
                                                 const unsigned long long* __restrict__ ws_in, uint32_t* __restrict__ jb_out,
                                                 uint32_t* __restrict__ hops_out, unsigned long long* __restrict__ ws_out,
                                                 unsigned long long* __restrict__ changed) {
    uint64_t c[1] = {0};
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        const uint32_t j = jb_in[e];
        if ((j & CT_DONE) || j >= n_edges) {   // (j >= n_edges without the bit cannot happen: links only take values of links)
            jb_out[e] = j;
            hops_out[e] = hops_in[e];
            ws_out[e] = ws_in[e];
            continue;
        }
        const uint32_t jj = jb_in[j];
        jb_out[e] = jj;
        hops_out[e] = hops_in[e] + hops_in[j];
        ws_out[e] = ws_in[e] + ws_in[j];
        c[0] += (jj & CT_DONE) != 0;
    }
    const uint64_t s = wave_sum64(c[0]);
    if (lane_id() == 0 && s) atomicAdd(changed, (unsigned long long)s);
}

// the head of the path that edge p lies on, CC_NONE where p reached none
__device__ inline uint32_t ct_head_of(uint32_t p, uint32_t n_edges, const uint8_t* __restrict__ cls, const uint32_t* __restrict__ jb) {
    if (p >= n_edges) return CC_NONE;
    if (cls[p] & CTC_START) return p;
    const uint32_t j = jb[p];
    return (j & CT_DONE) && (j & ~CT_DONE) < n_edges ? (j & ~CT_DONE) : CC_NONE;
}

__global__ __launch_bounds__(256) void k_ct_cover_init(const EdgeRanks* __restrict__ er, uint32_t n_edges, uint32_t n_order,
                                                       const uint32_t* __restrict__ ine, const uint8_t* __restrict__ cls,
                                                       const uint32_t* __restrict__ jb, uint32_t* __restrict__ cj, uint8_t* __restrict__ ok) {
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        const uint8_t k = cls[e];
        uint32_t link = e | CT_DONE;
        uint8_t good = 0;
        if ((k & CTC_START) && !(k & CTC_LATE)) {
            good = !(k & CTC_BLOCKED);
        } else if (k & CTC_START) {
            const uint32_t ru = er[e].ru;
            const uint32_t hd = ct_head_of(ru < n_order ? ine[ru] : CC_NONE, n_edges, cls, jb);
            if (hd != CC_NONE) {   // (else DEAD: final, never covered)
                const uint8_t hk = cls[hd];
                bool fin = !(hk & CTC_LATE), hok = fin && !(hk & CTC_BLOCKED);
                if (!fin) {        // a late start is final only when it is dead
                    const uint32_t hru = er[hd].ru;
                    fin = ct_head_of(hru < n_order ? ine[hru] : CC_NONE, n_edges, cls, jb) == CC_NONE;
                }
                link = fin ? (hd | CT_DONE) : hd;
                good = !(k & CTC_BLOCKED) && (!fin || hok);
            }
        }
        cj[e] = link;   // (an extension: final and 0, never read)
        ok[e] = good;
    }
}

__global__ __launch_bounds__(256) void k_ct_cover_jump(uint32_t n_edges, const uint32_t* __restrict__ cj_in, const uint8_t* __restrict__ ok_in,
                                                       uint32_t* __restrict__ cj_out, uint8_t* __restrict__ ok_out,
                                                       unsigned long long* __restrict__ changed) {
    uint64_t c[1] = {0};
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        const uint32_t j = cj_in[e];
        if ((j & CT_DONE) || j >= n_edges) {
            cj_out[e] = j;
            ok_out[e] = ok_in[e];
            continue;
        }
        const uint32_t jj = cj_in[j];
        cj_out[e] = jj;
        ok_out[e] = ok_in[e] & ok_in[j];
        c[0] += (jj & CT_DONE) != 0;
    }
    const uint64_t s = wave_sum64(c[0]);
    if (lane_id() == 0 && s) atomicAdd(changed, (unsigned long long)s);
}

__global__ __launch_bounds__(256) void k_ct_paths(const EdgeRanks* __restrict__ er, const Edge* __restrict__ edges, uint32_t n_edges,
                                                  uint32_t n_order, const uint32_t* __restrict__ indeg, const uint32_t* __restrict__ outdeg,
                                                  const long long* __restrict__ nlen, const uint8_t* __restrict__ cls,
                                                  const uint32_t* __restrict__ jb, const uint32_t* __restrict__ hops,
                                                  const unsigned long long* __restrict__ ws, const uint32_t* __restrict__ cj,
                                                  const uint8_t* __restrict__ ok, uint32_t* __restrict__ head_of, uint32_t* __restrict__ pn,
                                                  uint32_t* __restrict__ plast, long long* __restrict__ plen,
                                                  unsigned long long* __restrict__ counters) {
    uint64_t c[2] = {0, 0};   // covered, uncovered
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        const EdgeRanks x = er[e];
        const uint32_t hd = x.ru < n_order && x.rv < n_order ? ct_head_of(e, n_edges, cls, jb) : CC_NONE;
        const bool covered = hd != CC_NONE && (cj[hd] & CT_DONE) && ok[hd];
        head_of[e] = covered ? hd : CC_NONE;
        c[0] += covered;
        c[1] += !covered;
        if (!covered || (indeg[x.rv] == 1 && outdeg[x.rv] == 1)) continue;
        const bool start = hd == e;   // the path's last edge: one per head
        pn[hd] = (start ? 0u : hops[e]) + 2u;
        plast[hd] = x.rv;
        plen[hd] = (long long)((unsigned long long)(long long)edges[hd].weight + (start ? 0ull : ws[e]) + (unsigned long long)nlen[x.rv]);
    }
    block_add<2>(c, counters + TK_COVERED);
}
static_assert(TK_UNCOVERED == TK_COVERED + 1, "k_ct_paths adds the two in one go");

__global__ __launch_bounds__(256) void k_ct_filter(uint32_t n_edges, unsigned long long min_len, const uint32_t* __restrict__ head_of,
                                                   const uint32_t* __restrict__ pn, const long long* __restrict__ plen,
                                                   uint8_t* __restrict__ kept, unsigned long long* __restrict__ counters) {
    uint64_t c[4] = {0, 0, 0, 0};   // paths, short ones, kept ones, the edges of all paths
    unsigned long long mx = 0;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        const bool head = head_of[e] == e;
        bool keep = false;
        if (head) {
            const uint32_t nodes = pn[e];
            if (nodes < 2 || nodes > n_edges + 1) {   // (no last edge wrote here: an error on the host)
                atomicAdd(&counters[TK_BAD], 1ull);
            } else {
                keep = ct_long_enough(plen[e], min_len);
                ++c[0];
                c[1] += !keep;
                c[2] += keep;
                c[3] += nodes - 1;
                mx = nodes > mx ? nodes : mx;
            }
        }
        kept[e] = keep;
    }
    block_add<4>(c, counters + TK_PATHS);
    if (mx) atomicMax(&counters[TK_MAXN], mx);
}
static_assert(TK_SHORT == TK_PATHS + 1 && TK_KEPT == TK_PATHS + 2 && TK_PEDGES == TK_PATHS + 3, "k_ct_filter adds the four in one go");

__global__ __launch_bounds__(256) void k_ct_isolated(uint32_t n_order, unsigned long long min_len, const uint32_t* __restrict__ indeg,
                                                     const uint32_t* __restrict__ outdeg, const long long* __restrict__ nlen,
                                                     uint8_t* __restrict__ root, unsigned long long* __restrict__ counters) {
    uint64_t c[2] = {0, 0};   // isolated, short ones
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        const bool iso = indeg[r] == 0 && outdeg[r] == 0, keep = iso && ct_long_enough(nlen[r], min_len);
        root[r] = keep;
        c[0] += iso;
        c[1] += iso && !keep;
    }
    block_add<2>(c, counters + TK_ISO);
}
static_assert(TK_SHORTISO == TK_ISO + 1, "k_ct_isolated adds the two in one go");

// the sort's input: (rank of the first node, edge) of every surviving head at its place among them, all ones behind
__global__ __launch_bounds__(256) void k_ct_keys(const EdgeRanks* __restrict__ er, uint32_t n_edges, uint32_t n_kept, uint32_t n_pad,
                                                 const uint8_t* __restrict__ kept, const uint32_t* __restrict__ eidx,
                                                 unsigned long long* __restrict__ key, uint32_t* __restrict__ val) {
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges || e < n_pad; e += gridDim.x * blockDim.x) {
        if (e >= n_kept && e < n_pad) {
            key[e] = ~0ull;
            val[e] = CC_NONE;
        }
        if (e < n_edges && kept[e]) {
            const uint32_t i = eidx[e];
            if (i >= n_kept) continue;   // (cannot happen: the prefix sum counted this edge)
            key[i] = ((unsigned long long)er[e].ru << 32) | e;
            val[i] = e;
        }
    }
}

__global__ __launch_bounds__(256) void k_ct_number(const EdgeRanks* __restrict__ er, uint32_t n_edges, uint32_t n_order, uint32_t n_kept,
                                                   const uint32_t* __restrict__ val, const uint32_t* __restrict__ node_at,
                                                   const uint32_t* __restrict__ pn, const uint32_t* __restrict__ plast,
                                                   const long long* __restrict__ plen, uint32_t* __restrict__ cidx,
                                                   Contig* __restrict__ table) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_kept; i += gridDim.x * blockDim.x) {
        const uint32_t e = val[i];
        if (e >= n_edges) continue;   // (cannot happen: the first n_kept places hold the surviving heads)
        cidx[e] = i;
        const uint32_t ru = er[e].ru, rl = plast[e];
        table[i] = Contig{ru < n_order ? node_at[ru] : CC_NONE, rl < n_order ? node_at[rl] : CC_NONE, pn[e], e, plen[e]};
    }
}

__global__ __launch_bounds__(256) void k_ct_iso_table(uint32_t n_order, uint32_t n_kept, uint32_t n_iso, const uint8_t* __restrict__ root,
                                                      const uint32_t* __restrict__ index, const uint32_t* __restrict__ node_at,
                                                      const long long* __restrict__ nlen, Contig* __restrict__ table) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        if (!root[r]) continue;
        const uint32_t i = index[r];
        if (i >= n_iso) continue;   // (cannot happen: the prefix sum counted this rank)
        table[n_kept + i] = Contig{node_at[r], node_at[r], 1u, CC_NONE, nlen[r]};
    }
}

__global__ __launch_bounds__(256) void k_ct_edge_out(uint32_t n_edges, const uint32_t* __restrict__ head_of, const uint8_t* __restrict__ kept,
                                                     const uint32_t* __restrict__ cidx, const uint32_t* __restrict__ hops,
                                                     uint32_t* __restrict__ contig_out, uint32_t* __restrict__ pos_out) {
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        const uint32_t hd = head_of[e];
        const bool on = hd < n_edges && kept[hd];
        contig_out[e] = on ? cidx[hd] : CC_NONE;
        pos_out[e] = on ? (hd == e ? 0u : hops[e]) : CC_NONE;
    }
}

}  // namespace po
