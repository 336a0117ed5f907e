// Device side of the relevant reads of `phasm phase`: the alignment map and, per bubble, what
//   _get_read_alignments                                   phasm/cli/assembler.py:313-328
//   get_aligning_reads                                     phasm/phasing.py:541-550
//   the spanning-read intersection                         phasm/phasing.py:263-286
//   get_relevant_read_info / _get_max_possible_overlap     phasm/phasing.py:366-419
// compute, in the layout po_phase_branch takes (phase.hip.h).
//
// THE INDEX (po_phase_index).  Row i = (a, b, astart, aend, bstart, bend) writes m[a][b] = (astart, aend) with sequence
// number 2i, then m[b][a] = (bstart, bend) with 2i + 1; the entry of a key is the write with the greatest number.
//   k_rr_insert   both writes of every row: the key (x << 32 | y) into an open-addressing table of 64-bit keys (load <= 0.5,
//                 multiply-shift slot, as coverage.hip.h) by a CAS claim, then an integer atomicMax of the sequence number on
//                 the slot's value word.  The ONE lane that claims a slot counts the key for x.
//   k_rr_degree   the largest segment
//   k_rr_fill     (after a prefix sum of the counts) every occupied slot reads the winning row again and writes
//                 {y, a0, a1, seq} into the segment of x, in the order the slots come -- which is free
//   k_rr_sort     the segments into ascending y, PER SEGMENT and by rank: entry j of a segment goes to the place given by the
//                 number of entries of its segment with a smaller y (the keys of a segment are distinct, so the ranks are a
//                 permutation).  One thread per entry, the segment read from global memory: there is no LDS tile, so a
//                 segment of any size takes this one path -- at d entries d * d comparisons, d at a time.
//   k_rr_place    the place of every entry into the value word of its slot: a point look-up (x, y) is one probe sequence
//                 and one entry
// Two runs give the same bytes: the winner is decided by integers, the places by the sort.
// Memory of an index: 12 bytes per slot (4 slots per row: 48 bytes per row), 16 per key (at most 2 per row: 32 bytes per
// row), 8 per read (offsets, lengths) -- at most 80 bytes per row + 8 per read; while it is built another 20 per key (the
// unsorted entries and their x) and 8 per read.
//
// THE GATHER (po_phase_relevant), on bitsets of W = ceil(n_ids / 32) words over the read ids:
//   k_rr_mark       the ids of a list into a bitset (atomicOr on words; duplicates set a bit twice)
//   k_rr_mark_seg   one wave per cur_graph read: the y of its segment into cur_aligning
//   k_rr_count      |cur_aligning| and |prev_aligning & cur_aligning|
//   k_rr_select     per word: the relevant reads (cur_aligning, or the intersection), G = cur_graph | prev_graph (or
//                   cur_graph alone after the fallback), and the popcounts of cur_aligning, relevant and G
//   k_rr_list       (after a prefix sum of the popcounts) a bitset as an ascending list; the same sums make local(y) a rank
//                   query: rank[y / 32] + popcount of the lower bits
//   k_rr_alncount   one wave per relevant read: its entries with y in G
//   k_rr_alnwrite   (after a prefix sum) those entries as (local(y), a0, a1), in segment order = ascending y
//   k_rr_omax       one thread per relevant read: min(len, pred_edge_len[p] - a0(p, r)) over the given preds, by table look-up
// Work per call: the segments of cur_graph and of the relevant reads, plus a few passes over W words.  Integers only; every
// probe loop is bounded by the table size, every other loop by a count.
#pragma once

namespace po {

enum { RX_INVALID = 0, RX_KEYS = 1, RX_MAXDEG = 2, RX_N = 3 };
enum { RG_CA = 0, RG_SPAN = 1, RG_N = 2 };
constexpr unsigned long long RR_EMPTY = ~0ull;   // (a read id is below 2^32 - 1: no key is all ones)
constexpr uint32_t RR_NO_SLOT = 0xFFFFFFFFu;

struct RrEntry {   // = po_alignment
    uint32_t b;
    int32_t a0, a1;
    uint32_t seq;
};

// slots of the key table for n_rows rows: at most 2 * n_rows keys (below 2^31), load <= 0.5, indexed with 32 bits
inline uint32_t rr_table_slots(uint64_t n_rows) {
    const uint64_t want = 4 * n_rows + 64;
    return want > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)want;
}

__device__ inline uint32_t rr_slot(unsigned long long key, uint32_t n_slots) {
    const unsigned long long k = key * 0x9E3779B97F4A7C15ull;
    return (uint32_t)(((k >> 32) * (unsigned long long)n_slots) >> 32);
}

// the slot of a key, RR_NO_SLOT when the table does not hold it
__device__ inline uint32_t rr_find(const unsigned long long* __restrict__ table, uint32_t n_slots, unsigned long long key) {
    uint32_t s = rr_slot(key, n_slots);
    for (uint32_t probe = 0; probe < n_slots; ++probe) {
        const unsigned long long k = table[s];
        if (k == key) return s;
        if (k == RR_EMPTY) return RR_NO_SLOT;
        s = s + 1 == n_slots ? 0 : s + 1;
    }
    return RR_NO_SLOT;
}

// the slot of a key that is claimed if no one has; `mine` for the one caller that found it empty
__device__ inline uint32_t rr_claim(unsigned long long* __restrict__ table, uint32_t n_slots, unsigned long long key, bool& mine) {
    uint32_t s = rr_slot(key, n_slots);
    mine = false;
    for (uint32_t probe = 0; probe < n_slots; ++probe) {
        const unsigned long long old = atomicCAS(&table[s], RR_EMPTY, key);
        if (old == RR_EMPTY) {
            mine = true;
            return s;
        }
        if (old == key) return s;
        s = s + 1 == n_slots ? 0 : s + 1;
    }
    return RR_NO_SLOT;   // (cannot happen: the table holds more slots than there can be keys)
}

__device__ inline bool rr_bit(const uint32_t* __restrict__ bits, uint32_t id) { return (bits[id >> 5] >> (id & 31)) & 1u; }

__global__ __launch_bounds__(256) void k_rr_insert(const Row* __restrict__ rows, uint32_t n_rows, uint32_t n_ids,
                                                   unsigned long long* __restrict__ table, uint32_t* __restrict__ tval, uint32_t n_slots,
                                                   uint32_t* __restrict__ deg, unsigned long long* __restrict__ counters) {
    uint64_t c[2] = {0, 0};   // rows that name a read the handle does not hold, keys
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_rows; i += gridDim.x * blockDim.x) {
        const uint32_t a = rows[i].a_idx, b = rows[i].b_idx;
        if (a >= n_ids || b >= n_ids) {
            c[0] += 1;
            continue;
        }
#pragma unroll
        for (uint32_t dir = 0; dir < 2; ++dir) {
            const uint32_t x = dir ? b : a, y = dir ? a : b;
            bool mine;
            const uint32_t s = rr_claim(table, n_slots, ((unsigned long long)x << 32) | y, mine);
            if (s == RR_NO_SLOT) continue;
            if (mine) {
                atomicAdd(&deg[x], 1u);
                c[1] += 1;
            }
            atomicMax(&tval[s], 2u * i + dir);   // (the value words start at 0; 2 * n_rows < 2^31)
        }
    }
    const uint64_t s0 = wave_sum64(c[0]);
    if (lane_id() == 0 && s0) atomicAdd(&counters[RX_INVALID], (unsigned long long)s0);
    const uint64_t s1 = wave_sum64(c[1]);
    if (lane_id() == 0 && s1) atomicAdd(&counters[RX_KEYS], (unsigned long long)s1);
}

__global__ __launch_bounds__(256) void k_rr_degree(const uint32_t* __restrict__ deg, uint32_t n_ids, unsigned long long* __restrict__ counters) {
    uint32_t m = 0;
    for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n_ids; x += gridDim.x * blockDim.x) m = deg[x] > m ? deg[x] : m;
    if (m) atomicMax(&counters[RX_MAXDEG], (unsigned long long)m);
}

__global__ __launch_bounds__(256) void k_rr_fill(const unsigned long long* __restrict__ table, const uint32_t* __restrict__ tval,
                                                 uint32_t n_slots, const Row* __restrict__ rows, uint32_t n_rows, uint32_t n_ids,
                                                 const uint32_t* __restrict__ off, uint32_t* __restrict__ cur, RrEntry* __restrict__ tmp,
                                                 uint32_t* __restrict__ ex, uint32_t n_keys) {
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < n_slots; s += gridDim.x * blockDim.x) {
        const unsigned long long k = table[s];
        if (k == RR_EMPTY) continue;
        const uint32_t x = (uint32_t)(k >> 32), seq = tval[s], i = seq >> 1;
        if (x >= n_ids || i >= n_rows) continue;   // (never index on trust)
        const Row r = rows[i];
        const uint32_t at = off[x] + atomicAdd(&cur[x], 1u);
        if (at >= n_keys) continue;
        tmp[at] = (seq & 1u) ? RrEntry{(uint32_t)k, r.bstart, r.bend, seq} : RrEntry{(uint32_t)k, r.astart, r.aend, seq};
        ex[at] = x;
    }
}

__global__ __launch_bounds__(256) void k_rr_sort(const RrEntry* __restrict__ tmp, const uint32_t* __restrict__ ex,
                                                 const uint32_t* __restrict__ off, uint32_t n_keys, uint32_t n_ids,
                                                 RrEntry* __restrict__ out) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n_keys; j += gridDim.x * blockDim.x) {
        const uint32_t x = ex[j];
        if (x >= n_ids) continue;
        const uint32_t base = off[x], end = off[x + 1];
        if (j < base || j >= end || end > n_keys) continue;
        const RrEntry mine = tmp[j];
        uint32_t rank = 0;
        for (uint32_t i = base; i < end; ++i) rank += tmp[i].b < mine.b;
        out[base + rank] = mine;
    }
}

__global__ __launch_bounds__(256) void k_rr_place(const RrEntry* __restrict__ entries, const uint32_t* __restrict__ ex, uint32_t n_keys,
                                                  const unsigned long long* __restrict__ table, uint32_t* __restrict__ tval,
                                                  uint32_t n_slots) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n_keys; j += gridDim.x * blockDim.x) {
        // (ex[j] is the x of the whole segment that place j lies in, sorted or not)
        const uint32_t s = rr_find(table, n_slots, ((unsigned long long)ex[j] << 32) | entries[j].b);
        if (s != RR_NO_SLOT) tval[s] = j;
    }
}

// ---- the gather ---------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_rr_mark(const uint32_t* __restrict__ list, uint32_t n, uint32_t n_ids, uint32_t* __restrict__ bits) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t id = list[i];
        if (id < n_ids) atomicOr(&bits[id >> 5], 1u << (id & 31));   // (the host refused ids at or above n_ids)
    }
}

__global__ __launch_bounds__(256) void k_rr_mark_seg(const uint32_t* __restrict__ cur, uint32_t n_cur, uint32_t n_ids,
                                                     const uint32_t* __restrict__ off, const RrEntry* __restrict__ entries, uint32_t n_keys,
                                                     uint32_t* __restrict__ ca) {
    const uint32_t n_waves = gridDim.x * blockDim.x / WAVE;
    for (uint32_t e = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE; e < n_cur; e += n_waves) {
        const uint32_t x = cur[e];
        if (x >= n_ids) continue;
        const uint32_t end = off[x + 1] < n_keys ? off[x + 1] : n_keys;
        for (uint32_t i = off[x] + lane_id(); i < end; i += WAVE) {
            const uint32_t y = entries[i].b;
            if (y < n_ids) atomicOr(&ca[y >> 5], 1u << (y & 31));
        }
    }
}

__global__ __launch_bounds__(256) void k_rr_count(const uint32_t* __restrict__ ca, const uint32_t* __restrict__ pa, uint32_t W,
                                                  unsigned long long* __restrict__ counters) {
    uint64_t c[2] = {0, 0};
    for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < W; w += gridDim.x * blockDim.x) {
        c[0] += (uint32_t)__popc(ca[w]);
        c[1] += (uint32_t)__popc(ca[w] & pa[w]);
    }
    const uint64_t s0 = wave_sum64(c[0]);
    if (lane_id() == 0 && s0) atomicAdd(&counters[RG_CA], (unsigned long long)s0);
    const uint64_t s1 = wave_sum64(c[1]);
    if (lane_id() == 0 && s1) atomicAdd(&counters[RG_SPAN], (unsigned long long)s1);
}

__global__ __launch_bounds__(256) void k_rr_select(const uint32_t* __restrict__ ca, const uint32_t* __restrict__ pa,
                                                   const uint32_t* __restrict__ gc, const uint32_t* __restrict__ gp, uint32_t W,
                                                   uint32_t use_pa, uint32_t use_prev, uint32_t* __restrict__ rel, uint32_t* __restrict__ g,
                                                   uint32_t* __restrict__ ca_cnt, uint32_t* __restrict__ rel_cnt, uint32_t* __restrict__ g_cnt) {
    for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < W; w += gridDim.x * blockDim.x) {
        const uint32_t r = use_pa ? ca[w] & pa[w] : ca[w], gg = use_prev ? gc[w] | gp[w] : gc[w];
        rel[w] = r;
        g[w] = gg;
        ca_cnt[w] = (uint32_t)__popc(ca[w]);
        rel_cnt[w] = (uint32_t)__popc(r);
        g_cnt[w] = (uint32_t)__popc(gg);
    }
}

__global__ __launch_bounds__(256) void k_rr_list(const uint32_t* __restrict__ bits, const uint32_t* __restrict__ rank, uint32_t W,
                                                 uint32_t* __restrict__ out, uint32_t cap) {
    for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < W; w += gridDim.x * blockDim.x) {
        const uint32_t v = bits[w];
        uint32_t at = rank[w];
        for (uint32_t b = 0; b < 32; ++b) {
            if (!((v >> b) & 1u)) continue;
            if (at < cap) out[at] = w * 32 + b;
            ++at;
        }
    }
}

__global__ __launch_bounds__(256) void k_rr_alncount(const uint32_t* __restrict__ rel_reads, uint32_t n_rel, uint32_t n_ids,
                                                     const uint32_t* __restrict__ off, const RrEntry* __restrict__ entries, uint32_t n_keys,
                                                     const uint32_t* __restrict__ g, uint32_t* __restrict__ aln_cnt) {
    const uint32_t n_waves = gridDim.x * blockDim.x / WAVE;
    for (uint32_t e = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE; e < n_rel; e += n_waves) {
        const uint32_t x = rel_reads[e];
        uint64_t mine = 0;
        if (x < n_ids) {
            const uint32_t end = off[x + 1] < n_keys ? off[x + 1] : n_keys;
            for (uint32_t i = off[x] + lane_id(); i < end; i += WAVE) {
                const uint32_t y = entries[i].b;
                mine += y < n_ids && rr_bit(g, y);
            }
        }
        const uint64_t all = wave_sum64(mine);
        if (lane_id() == 0) aln_cnt[e] = (uint32_t)all;
    }
}

__global__ __launch_bounds__(256) void k_rr_alnwrite(const uint32_t* __restrict__ rel_reads, uint32_t n_rel, uint32_t n_ids,
                                                     const uint32_t* __restrict__ off, const RrEntry* __restrict__ entries, uint32_t n_keys,
                                                     const uint32_t* __restrict__ g, const uint32_t* __restrict__ g_rank,
                                                     const uint32_t* __restrict__ aln_off, uint32_t n_aln, uint32_t* __restrict__ aln_b,
                                                     int32_t* __restrict__ aln_a0, int32_t* __restrict__ aln_a1) {
    const uint32_t n_waves = gridDim.x * blockDim.x / WAVE;
    for (uint32_t e = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE; e < n_rel; e += n_waves) {
        const uint32_t x = rel_reads[e];
        if (x >= n_ids) continue;
        const uint32_t base = off[x], end = off[x + 1] < n_keys ? off[x + 1] : n_keys;
        uint32_t at = aln_off[e];
        // (the whole wave takes every step: the ballot wants all lanes)
        for (uint32_t i0 = base; i0 < end; i0 += WAVE) {
            const uint32_t i = i0 + lane_id();
            RrEntry en = RrEntry{0, 0, 0, 0};
            bool in = false;
            if (i < end) {
                en = entries[i];
                in = en.b < n_ids && rr_bit(g, en.b);
            }
            const unsigned long long bal = __ballot(in);
            if (in) {
                const uint32_t to = at + (uint32_t)__popcll(bal & ((1ull << lane_id()) - 1ull));
                if (to < n_aln) {
                    aln_b[to] = g_rank[en.b >> 5] + (uint32_t)__popc(g[en.b >> 5] & ((1u << (en.b & 31)) - 1u));
                    aln_a0[to] = en.a0;
                    aln_a1[to] = en.a1;
                }
            }
            at += (uint32_t)__popcll(bal);
        }
    }
}

__global__ __launch_bounds__(256) void k_rr_omax(const uint32_t* __restrict__ rel_reads, uint32_t n_rel, uint32_t n_ids,
                                                 const uint32_t* __restrict__ len, const uint32_t* __restrict__ pred,
                                                 const int32_t* __restrict__ pred_len, uint32_t n_pred,
                                                 const unsigned long long* __restrict__ table, const uint32_t* __restrict__ tval,
                                                 uint32_t n_slots, const RrEntry* __restrict__ entries, uint32_t n_keys,
                                                 int32_t* __restrict__ omax) {
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_rel; e += gridDim.x * blockDim.x) {
        const uint32_t r = rel_reads[e];
        if (r >= n_ids) continue;
        long long om = (long long)len[r];
        for (uint32_t j = 0; j < n_pred; ++j) {
            const uint32_t s = rr_find(table, n_slots, ((unsigned long long)pred[j] << 32) | r);
            if (s == RR_NO_SLOT) continue;
            const uint32_t at = tval[s];
            if (at >= n_keys) continue;
            const long long v = (long long)pred_len[j] - (long long)entries[at].a0;
            om = v < om ? v : om;
        }
        omax[e] = (int32_t)om;
    }
}

}  // namespace po
