// Device side of the average coverage per edge of `phasm layout`:
//   average_coverage_path(g, read_alignments, [u, v])   phasm/assembly_graph.py:544-591, phasm/cli/assembler.py:190-193
// on an edge result (po_layout_edges, _reduce, _tips, _diamonds) or a merged graph (po_layout_merge) and ALL the rows.
//
// A(x) = the oriented reads that share a row with x, in either position.  Every oriented read is a member of at most one
// graph node (itself, or the merged path it lies on), so the distinct pairs (node, aligning read) number at most 2 * rows:
//   k_cov_mark / _nodes / _members   node_of[x]: x itself if an edge names it, n_ids + k for a member of merged path k whose
//                                    node has an edge, COV_NONE otherwise (contained reads, nodes without edges)
//   k_cov_insert                     both directions of every row: key (node_of[x], y) into an open-addressing table of
//                                    64-bit keys (load <= 0.5); the ONE lane that claims a slot adds len(y) to sum[node]
//                                    and counts the pair -- integer atomics only, the sums are the same on every run
//   k_cov_max                        the largest set
//   k_cov_fill                       (after a prefix sum of the counts) every occupied slot writes its read into the
//                                    segment of its node; the order inside a segment is free
//   k_cov_edges                      one wave per edge (u, v): sum[u] + sum[v] - the lengths of the reads of the SHORTER
//                                    list that the table also holds for the other node; u == v takes sum[u] alone;
//                                    path_length = weight + len(v) in 64 bits.  No float on the device.
// Every probe loop is bounded by the table size.
#pragma once

namespace po {

enum { CC_INVALID = 0, CC_NODES = 1, CC_PAIRS = 2, CC_MAXSET = 3, CC_ZERO = 4, CC_N = 5 };
constexpr uint32_t COV_NONE = 0xFFFFFFFFu;
constexpr unsigned long long COV_EMPTY = ~0ull;   // (a node id is below 2^32 - 1: no key is all ones)

struct EdgeCoverage {
    unsigned long long read_length_sum;
    long long path_length;
};

// slots of the pair table for n_rows rows: at most 2 * n_rows keys, load <= 0.5
inline uint32_t cov_table_slots(uint64_t n_rows) { return (uint32_t)(4 * n_rows + 64); }

// slot in [0, n_slots): multiply-shift range reduction, no power-of-two table needed
__device__ inline uint32_t cov_slot(unsigned long long key, uint32_t n_slots) {
    const unsigned long long k = key * 0x9E3779B97F4A7C15ull;
    return (uint32_t)(((k >> 32) * (unsigned long long)n_slots) >> 32);
}

__device__ inline bool cov_find(const unsigned long long* __restrict__ table, uint32_t n_slots, unsigned long long key) {
    uint32_t s = cov_slot(key, n_slots);
    for (uint32_t probe = 0; probe < n_slots; ++probe) {
        const unsigned long long k = table[s];
        if (k == key) return true;
        if (k == COV_EMPTY) return false;
        s = s + 1 == n_slots ? 0 : s + 1;
    }
    return false;
}

// used[n] = 1 for every node an edge names (n_total = reads + merged nodes)
__global__ __launch_bounds__(256) void k_cov_mark(const Edge* __restrict__ edges, uint32_t n_edges, uint32_t n_total,
                                                  uint32_t* __restrict__ used, unsigned long long* __restrict__ counters) {
    uint64_t c[1] = {0};
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
        const uint32_t u = edges[e].u, v = edges[e].v;
        if (u >= n_total || v >= n_total) {
            c[0] += 1;
            continue;
        }
        used[u] = 1;
        used[v] = 1;
    }
    const uint64_t s = wave_sum64(c[0]);
    if (lane_id() == 0 && s) atomicAdd(&counters[CC_INVALID], (unsigned long long)s);
}

// node_of of the reads that are nodes themselves; the nodes with an edge are counted
__global__ __launch_bounds__(256) void k_cov_nodes(uint32_t n_ids, uint32_t n_total, const uint32_t* __restrict__ used,
                                                   uint32_t* __restrict__ node_of, unsigned long long* __restrict__ counters) {
    uint64_t c[1] = {0};
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n < n_total) {
        const bool on = used[n] != 0;
        if (n < n_ids) node_of[n] = on ? n : COV_NONE;
        c[0] = on;
    }
    block_add<1>(c, counters + CC_NODES);
}

// node_of of the members of the merged paths: entry i of the member table belongs to the path k with off[k] <= i < off[k + 1]
__global__ __launch_bounds__(256) void k_cov_members(const uint32_t* __restrict__ member, uint32_t n_members,
                                                     const uint32_t* __restrict__ off, uint32_t n_paths, uint32_t n_ids,
                                                     const uint32_t* __restrict__ used, uint32_t* __restrict__ node_of,
                                                     unsigned long long* __restrict__ counters) {
    uint64_t c[1] = {0};
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_members && n_paths) {
        uint32_t lo = 0, hi = n_paths;   // off[lo] <= i < off[hi]  (off[n_paths] = n_members)
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (off[mid] <= i) lo = mid; else hi = mid;
        }
        const uint32_t m = member[i];
        if (m < n_ids) node_of[m] = used[n_ids + lo] ? n_ids + lo : COV_NONE; else c[0] = 1;
    }
    const uint64_t s = wave_sum64(c[0]);
    if (lane_id() == 0 && s) atomicAdd(&counters[CC_INVALID], (unsigned long long)s);
}

// the claim of one key; true for the one caller that found the slot empty
__device__ inline bool cov_claim(unsigned long long* __restrict__ table, uint32_t n_slots, unsigned long long key) {
    uint32_t s = cov_slot(key, n_slots);
    for (uint32_t probe = 0; probe < n_slots; ++probe) {
        const unsigned long long old = atomicCAS(&table[s], COV_EMPTY, key);
        if (old == COV_EMPTY) return true;
        if (old == key) return false;
        s = s + 1 == n_slots ? 0 : s + 1;
    }
    return false;   // (cannot happen: the table holds twice the keys there can be)
}

__global__ __launch_bounds__(256) void k_cov_insert(const Row* __restrict__ rows, uint32_t n_rows, uint32_t n_ids,
                                                    const uint32_t* __restrict__ len, const uint32_t* __restrict__ node_of,
                                                    unsigned long long* __restrict__ table, uint32_t n_slots,
                                                    unsigned long long* __restrict__ sum, uint32_t* __restrict__ cnt,
                                                    unsigned long long* __restrict__ counters) {
    uint64_t c[2] = {0, 0};   // rows that name a read the handle does not hold, pairs
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_rows; i += gridDim.x * blockDim.x) {
        const uint32_t a = rows[i].a_idx, b = rows[i].b_idx;
        if (a >= n_ids || b >= n_ids) {
            c[0] += 1;
            continue;
        }
#pragma unroll
        for (int dir = 0; dir < 2; ++dir) {
            const uint32_t x = dir ? b : a, y = dir ? a : b;
            if (dir && a == b) break;   // (a row (x, x): one pair)
            const uint32_t nd = node_of[x];
            if (nd == COV_NONE) continue;
            if (cov_claim(table, n_slots, ((unsigned long long)nd << 32) | y)) {
                atomicAdd(&sum[nd], (unsigned long long)len[y]);
                atomicAdd(&cnt[nd], 1u);
                c[1] += 1;
            }
        }
    }
    const uint64_t s = wave_sum64(c[0]);
    if (lane_id() == 0 && s) atomicAdd(&counters[CC_INVALID], (unsigned long long)s);
    const uint64_t p = wave_sum64(c[1]);
    if (lane_id() == 0 && p) atomicAdd(&counters[CC_PAIRS], (unsigned long long)p);
}

__global__ __launch_bounds__(256) void k_cov_max(const uint32_t* __restrict__ cnt, uint32_t n_total,
                                                 unsigned long long* __restrict__ counters) {
    uint32_t m = 0;
    for (uint32_t n = blockIdx.x * blockDim.x + threadIdx.x; n < n_total; n += gridDim.x * blockDim.x) m = cnt[n] > m ? cnt[n] : m;
    if (m) atomicMax(&counters[CC_MAXSET], (unsigned long long)m);
}

__global__ __launch_bounds__(256) void k_cov_fill(const unsigned long long* __restrict__ table, uint32_t n_slots, uint32_t n_total,
                                                  const uint32_t* __restrict__ off, uint32_t* __restrict__ cur,
                                                  uint32_t* __restrict__ list, uint32_t n_pairs) {
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < n_slots; s += gridDim.x * blockDim.x) {
        const unsigned long long k = table[s];
        if (k == COV_EMPTY) continue;
        const uint32_t nd = (uint32_t)(k >> 32);
        if (nd >= n_total) continue;   // (never index on trust)
        const uint32_t at = off[nd] + atomicAdd(&cur[nd], 1u);
        if (at < n_pairs) list[at] = (uint32_t)k;
    }
}

// One wave per edge.  The reference's `if include_last and last:` is false for a v of length 0 (a read's bool is its
// length): such a v adds neither its length nor its aligning reads.
__global__ __launch_bounds__(256) void k_cov_edges(const Edge* __restrict__ edges, uint32_t n_edges, uint32_t n_ids, uint32_t n_total,
                                                   const uint32_t* __restrict__ len, const long long* __restrict__ mlen,
                                                   const unsigned long long* __restrict__ table, uint32_t n_slots,
                                                   const unsigned long long* __restrict__ sum, const uint32_t* __restrict__ cnt,
                                                   const uint32_t* __restrict__ off, const uint32_t* __restrict__ list,
                                                   uint32_t n_pairs, EdgeCoverage* __restrict__ out,
                                                   unsigned long long* __restrict__ counters) {
    const uint32_t n_waves = gridDim.x * blockDim.x / WAVE;
    uint64_t zero = 0;
    for (uint32_t e = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE; e < n_edges; e += n_waves) {
        const Edge x = edges[e];
        if (x.u >= n_total || x.v >= n_total) continue;   // (counted by k_cov_mark: the call fails)
        const long long lv = x.v < n_ids ? (long long)len[x.v] : mlen[x.v - n_ids];
        unsigned long long s = sum[x.u];
        if (x.u != x.v && lv != 0) {
            const bool u_short = cnt[x.u] <= cnt[x.v];
            const uint32_t a = u_short ? x.u : x.v, b = u_short ? x.v : x.u;
            const uint32_t n = cnt[a], base = off[a];
            uint64_t both = 0;
            for (uint32_t i = lane_id(); i < n; i += WAVE) {
                if (base + i >= n_pairs) break;
                const uint32_t y = list[base + i];
                if (y < n_ids && cov_find(table, n_slots, ((unsigned long long)b << 32) | y)) both += len[y];
            }
            s = s + sum[x.v] - wave_sum64(both);
        }
        if (lane_id() == 0) {
            const long long path = (long long)x.weight + lv;
            out[e] = EdgeCoverage{s, path};
            zero += path == 0;
        }
    }
    if (zero) atomicAdd(&counters[CC_ZERO], (unsigned long long)zero);
}

}  // namespace po
