// Device side of the first step of superbubble detection inside `phasm chain`:
//   partition_graph(g)                                        phasm/bubbles.py:32-84
// on a graph result in HBM: the strongly connected components, the class of every edge and the flags that say where the
// reference adds its artificial 'r_' / 're_' edges.
//
// The scheme is trim + colouring on RANKS (the place of a node in the node order), with the rank machinery of
// components.hip.h unchanged (k_cc_keys / k_merge_bitonic / k_cc_init / k_cc_ends).  One live byte and one scc word per
// rank; scc[r] ends up as the lowest rank of r's SCC.
//   k_scc_init                                 live = 1, scc = none, marks clear
//   k_scc_trim_edges / k_scc_trim_ranks        per edge with both ends live and u != v: has_out[ru] = has_in[rv] = 1; per
//                                              live rank: a missing mark retires it as an SCC of its own.  Rounds, until
//                                              one removes nothing
//   k_scc_colour_init / k_scc_forward          colour[r] = r on the live ranks; per edge with both ends live:
//                                              atomicMin(&colour[rv], colour[ru]).  Rounds, until one lowers nothing:
//                                              colour[v] is then the lowest live rank that reaches v
//   k_scc_back_init / k_scc_backward           mark the roots (colour[r] == r); per edge with both ends live and of one
//                                              colour: a marked v marks u.  Rounds, until one marks nothing: the marked
//                                              ranks of colour c are the SCC of c
//   k_scc_retire                               marked: scc[r] = colour[r], live = 0
//   ... again from the trim rounds while live ranks remain (scc_drive below: the host bounds every loop).
//   k_scc_roots, a prefix sum, k_scc_label_nodes / k_scc_edges / k_scc_flags / k_scc_max
//                                              SCC i is the i-th in the order of each SCC's lowest rank; the table, the
//                                              class byte per edge, the flag byte per rank, the counts and maxima
// The colour words and mark bytes are READ with plain loads, which may see a word as it was earlier in the same launch:
// an older colour is a higher one, an older mark is 0, so a round only does less with them, never wrong (a mark seen as 0
// stores the 1 again); the round that ends a loop wrote nothing, so it read everything as it is.  Colours are WRITTEN by
// atomicMin only, bytes by plain stores of one value.  Integer atomics only: every output is the same on every run.
#pragma once

namespace po {

enum { PC_INVALID = 0, PC_ORDER = 1,   // (k_cc_ends and k_cc_init count into these two: KC_INVALID, KC_ORDER)
       PC_SINGLE = 2, PC_MAXN = 3, PC_MAXE = 4, PC_SELF = 5, PC_CLASS = 6 /* .. 10 */, PC_N = 11 };
static_assert(PC_INVALID == KC_INVALID && PC_ORDER == KC_ORDER, "the rank kernels of components.hip.h count into the same words");

enum : uint32_t { SF_R_IN = 1, SF_RE_OUT = 2, SF_START = 4, SF_SINK = 8, SF_HAS_IN = 16, SF_HAS_OUT = 32 };   // (the last two: work bits)

struct Scc {
    uint32_t first_node, n_nodes;
    unsigned long long n_edges;
    uint32_t n_r_in, n_re_out;
};

struct SccWork {
    uint64_t n_trimmed = 0;
    uint32_t outer = 0, trim_rounds = 0, forward_rounds = 0, backward_rounds = 0, batches = 0;
};

enum { SCC_DONE = ROUNDS_DONE, SCC_ROUND_CAP = ROUNDS_CAP, SCC_OUTER_CAP = 2, SCC_FAILED = ROUNDS_FAILED, SCC_STUCK = 4 };

// The whole loop.  Ops launches (trim_round, colour_init, forward_round, back_init, backward_round take the index of the
// round's change word) and reads back (begin / end, retire).  Every outer iteration retires at least its lowest live rank,
// so there are at most n_order of them.  A phase is one round_phase (components.hip.h) on the ranks live at its start: its
// words are final after at most `live` rounds (every round but the last removes, lowers along one more edge of a shortest
// path, or marks at least one rank), the round after that counts nothing.
template <class Ops>
inline int scc_drive(Ops& ops, uint64_t n_order, SccWork& w) {
    uint64_t live = n_order;
    while (live) {
        if (w.outer >= n_order) return SCC_OUTER_CAP;
        ++w.outer;
        uint64_t trimmed = 0, ignored = 0, retired = 0;
        int s = round_phase(ops, live, [&](uint32_t j) { ops.trim_round(j); }, w.trim_rounds, w.batches, trimmed);
        if (s != SCC_DONE) return s;
        if (trimmed > live) return SCC_STUCK;
        w.n_trimmed += trimmed;
        live -= trimmed;
        if (!live) break;
        ops.colour_init();
        s = round_phase(ops, live, [&](uint32_t j) { ops.forward_round(j); }, w.forward_rounds, w.batches, ignored);
        if (s != SCC_DONE) return s;
        ops.back_init();
        s = round_phase(ops, live, [&](uint32_t j) { ops.backward_round(j); }, w.backward_rounds, w.batches, ignored);
        if (s != SCC_DONE) return s;
        if (!ops.retire(retired)) return SCC_FAILED;
        if (retired == 0 || retired > live) return SCC_STUCK;
        live -= retired;
    }
    return SCC_DONE;
}

__global__ __launch_bounds__(256) void k_scc_init(uint32_t n_order, uint8_t* __restrict__ live, uint32_t* __restrict__ scc,
                                                  uint8_t* __restrict__ has_in, uint8_t* __restrict__ has_out) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        live[r] = 1;
        scc[r] = CC_NONE;
        has_in[r] = has_out[r] = 0;
    }
}

__global__ __launch_bounds__(256) void k_scc_trim_edges(const EdgeRanks* __restrict__ er, uint32_t n_edges, uint32_t n_order,
                                                        const uint8_t* __restrict__ live, uint8_t* __restrict__ has_in,
                                                        uint8_t* __restrict__ has_out) {
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        const EdgeRanks x = er[e];
        if (x.ru >= n_order || x.rv >= n_order || x.ru == x.rv) continue;   // (a self-loop keeps nothing alive)
        if (!live[x.ru] || !live[x.rv]) continue;
        has_out[x.ru] = 1;
        has_in[x.rv] = 1;
    }
}

__global__ __launch_bounds__(256) void k_scc_trim_ranks(uint32_t n_order, uint8_t* __restrict__ live, uint32_t* __restrict__ scc,
                                                        uint8_t* __restrict__ has_in, uint8_t* __restrict__ has_out,
                                                        unsigned long long* __restrict__ removed) {
    uint64_t c[1] = {0};
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        const bool both = has_in[r] && has_out[r];
        has_in[r] = has_out[r] = 0;
        if (live[r] && !both) {
            scc[r] = r;
            live[r] = 0;
            ++c[0];
        }
    }
    const uint64_t s = wave_sum64(c[0]);
    if (lane_id() == 0 && s) atomicAdd(removed, (unsigned long long)s);
}

__global__ __launch_bounds__(256) void k_scc_colour_init(uint32_t n_order, const uint8_t* __restrict__ live,
                                                         uint32_t* __restrict__ colour, uint8_t* __restrict__ mark) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        colour[r] = live[r] ? r : CC_NONE;
        mark[r] = 0;
    }
}

__global__ __launch_bounds__(256) void k_scc_forward(const EdgeRanks* __restrict__ er, uint32_t n_edges, uint32_t n_order,
                                                     const uint8_t* __restrict__ live, uint32_t* __restrict__ colour,
                                                     unsigned long long* __restrict__ changed) {
    uint64_t c[1] = {0};
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        const EdgeRanks x = er[e];
        if (x.ru >= n_order || x.rv >= n_order || x.ru == x.rv) continue;
        if (!live[x.ru] || !live[x.rv]) continue;
        const uint32_t cu = colour[x.ru];
        if (cu < colour[x.rv]) c[0] += atomicMin(&colour[x.rv], cu) > cu;
    }
    const uint64_t s = wave_sum64(c[0]);
    if (lane_id() == 0 && s) atomicAdd(changed, (unsigned long long)s);
}

__global__ __launch_bounds__(256) void k_scc_back_init(uint32_t n_order, const uint8_t* __restrict__ live,
                                                       const uint32_t* __restrict__ colour, uint8_t* __restrict__ mark) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x)
        mark[r] = live[r] && colour[r] == r;
}

__global__ __launch_bounds__(256) void k_scc_backward(const EdgeRanks* __restrict__ er, uint32_t n_edges, uint32_t n_order,
                                                      const uint8_t* __restrict__ live, const uint32_t* __restrict__ colour,
                                                      uint8_t* __restrict__ mark, unsigned long long* __restrict__ changed) {
    uint64_t c[1] = {0};
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        const EdgeRanks x = er[e];
        if (x.ru >= n_order || x.rv >= n_order || x.ru == x.rv) continue;
        if (!live[x.ru] || !live[x.rv] || colour[x.ru] != colour[x.rv]) continue;
        if (mark[x.rv] && !mark[x.ru]) {
            mark[x.ru] = 1;   // (every writer stores the same value)
            ++c[0];
        }
    }
    const uint64_t s = wave_sum64(c[0]);
    if (lane_id() == 0 && s) atomicAdd(changed, (unsigned long long)s);
}

__global__ __launch_bounds__(256) void k_scc_retire(uint32_t n_order, uint8_t* __restrict__ live, const uint32_t* __restrict__ colour,
                                                    const uint8_t* __restrict__ mark, uint32_t* __restrict__ scc,
                                                    unsigned long long* __restrict__ retired) {
    uint64_t c[1] = {0};
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        if (!live[r] || !mark[r]) continue;
        scc[r] = colour[r];
        live[r] = 0;
        ++c[0];
    }
    const uint64_t s = wave_sum64(c[0]);
    if (lane_id() == 0 && s) atomicAdd(retired, (unsigned long long)s);
}

__global__ __launch_bounds__(256) void k_scc_roots(const uint32_t* __restrict__ scc, uint32_t n_order, uint8_t* __restrict__ root,
                                                   uint32_t* __restrict__ flagw) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        root[r] = scc[r] == r;
        flagw[r] = 0;
    }
}

__global__ __launch_bounds__(256) void k_scc_label_nodes(const uint32_t* __restrict__ scc, const uint32_t* __restrict__ index,
                                                         const uint32_t* __restrict__ node_at, uint32_t n_order, uint32_t n_scc,
                                                         uint32_t* __restrict__ node_scc, Scc* __restrict__ table) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        const uint32_t q = scc[r];
        const uint32_t c = q < n_order ? index[q] : CC_NONE;
        if (c >= n_scc) {   // (cannot happen once every rank is retired)
            node_scc[r] = CC_NONE;
            continue;
        }
        node_scc[r] = c;
        atomicAdd(&table[c].n_nodes, 1u);
        if (q == r) table[c].first_node = node_at[r];
    }
}

// the class of every edge (a launch of its own: it reads the finished n_nodes of the table), the edges inside each SCC,
// and per end the bits the flags come from
__global__ __launch_bounds__(256) void k_scc_edges(const EdgeRanks* __restrict__ er, uint32_t n_edges, uint32_t n_order, uint32_t n_scc,
                                                   const uint32_t* __restrict__ node_scc, Scc* __restrict__ table,
                                                   uint8_t* __restrict__ edge_class, uint32_t* __restrict__ flagw,
                                                   unsigned long long* __restrict__ counters) {
    uint64_t c[6] = {0, 0, 0, 0, 0, 0};   // self-loops, then the five classes
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        const EdgeRanks x = er[e];
        const uint32_t cu = x.ru < n_order ? node_scc[x.ru] : CC_NONE, cv = x.rv < n_order ? node_scc[x.rv] : CC_NONE;
        if (cu >= n_scc || cv >= n_scc) {
            edge_class[e] = 0xFF;
            continue;
        }
        const bool su = table[cu].n_nodes == 1, sv = table[cv].n_nodes == 1;
        uint32_t k, bu = SF_HAS_OUT, bv = SF_HAS_IN;
        if (cu == cv) {
            k = su ? 1 : 0;
            atomicAdd(&table[cu].n_edges, 1ull);
        } else {
            k = su ? (sv ? 1 : 2) : (sv ? 3 : 4);
        }
        if (k >= 2) {   // the edge leaves one partition and enters another
            bu |= SF_RE_OUT;
            bv |= SF_R_IN;
        }
        edge_class[e] = (uint8_t)k;
        if ((flagw[x.ru] & bu) != bu) atomicOr(&flagw[x.ru], bu);
        if ((flagw[x.rv] & bv) != bv) atomicOr(&flagw[x.rv], bv);
        c[0] += x.ru == x.rv;
        c[1] += k == 0;
        c[2] += k == 1;
        c[3] += k == 2;
        c[4] += k == 3;
        c[5] += k == 4;
    }
    block_add<6>(c, counters + PC_SELF);
}
static_assert(PC_CLASS == PC_SELF + 1, "k_scc_edges adds self-loops and the five classes in one go");

__global__ __launch_bounds__(256) void k_scc_flags(uint32_t n_order, uint32_t n_scc, const uint32_t* __restrict__ node_scc,
                                                   const uint32_t* __restrict__ flagw, Scc* __restrict__ table,
                                                   uint8_t* __restrict__ flags) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        const uint32_t c = node_scc[r], w = flagw[r];
        if (c >= n_scc) {
            flags[r] = 0xFF;
            continue;
        }
        uint32_t f = w & (SF_R_IN | SF_RE_OUT);
        if (table[c].n_nodes == 1) f |= (w & SF_HAS_IN ? 0 : SF_START) | (w & SF_HAS_OUT ? 0 : SF_SINK);
        flags[r] = (uint8_t)f;
        if (f & SF_R_IN) atomicAdd(&table[c].n_r_in, 1u);
        if (f & SF_RE_OUT) atomicAdd(&table[c].n_re_out, 1u);
    }
}

__global__ __launch_bounds__(256) void k_scc_max(const Scc* __restrict__ table, uint32_t n_scc, unsigned long long* __restrict__ counters) {
    uint64_t single = 0;
    unsigned long long mn = 0, me = 0;
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < n_scc; c += gridDim.x * blockDim.x) {
        const uint32_t nn = table[c].n_nodes;
        const unsigned long long ne = table[c].n_edges;
        single += nn == 1;
        mn = nn > mn ? nn : mn;
        me = ne > me ? ne : me;
    }
    const uint64_t s = wave_sum64(single);
    if (lane_id() == 0 && s) atomicAdd(&counters[PC_SINGLE], (unsigned long long)s);
    if (mn) atomicMax(&counters[PC_MAXN], mn);
    if (me) atomicMax(&counters[PC_MAXE], me);
}

}  // namespace po
