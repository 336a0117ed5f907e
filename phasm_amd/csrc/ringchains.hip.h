// Device side of the RING CHAINS of `phasm chain`: what po_layout_bubblechains_all and
// po_layout_contigs_all add to the bubble-chain stage of bubblechains.hip.h, whose kernels run unchanged around these.
//
// Behind po_layout_superbubbles_all's stage the links of the top-level bubbles are no forest of paths any more: a node still
// enters at most one top-level bubble and exits at most one, so the links form disjoint PATHS and RINGS.  On a ring every
// entrance has a pred, k_bc_heads finds no head and the ranking of k_bc_jump has nowhere to settle.  The kernels here elect
// one LEADER per ring, its lowest-ranked entrance, and cut the ranking's start there; k_bc_jump / k_bc_place then rank the
// ring as a path from its leader.
//   k_rc_init                                  per rank: ptr = the ranking's start of k_bc_heads (pred of a linked top-level
//                                              entrance, else the rank itself), mn = the rank
//   k_rc_round                                 mn = min(mn, mn[ptr]); ptr = ptr[ptr], from one buffer pair into the other
//                                              (in place a word that the same launch has already doubled would be doubled
//                                              again).  After k rounds mn covers the 2^k entrances from r backwards and ptr
//                                              is the entrance 2^k links back, or the head where the path ends sooner.  The
//                                              host launches exactly ceil(log2(n_top)) + 1 rounds: 2^k >= 2 n_top, so ptr
//                                              has reached the head of every path and mn has covered every ring whole
//   k_rc_leaders                               a top-level entrance whose ptr is no head lies on a ring; the one with
//                                              mn == r is its leader: BCW_HEAD and RCW_RING, the ranking's start cut to
//                                              (r, 0), +1 head, +1 ring.  Only the leader's own thread writes a word of its
//                                              ring, and it reads its own word before it writes
//   k_rc_close                                 behind k_bc_place: a ring has no entrance without next, so nothing stored the
//                                              last exit; last[leader] = leader.  The bubbles of all rings for the stats
// No kernel follows links in a loop and nothing is read back between the rounds: their number is fixed by the host.
// Integer atomics only: every output is the same on every run.
#pragma once

namespace po {

// counters behind those of bubblechains.hip.h, in the same 16 words
enum { HKR_RINGS = HK_N, HKR_RBUBBLES = HK_N + 1, HKR_N = HK_N + 2 };
static_assert(HKR_N <= 16, "the counters of the bubble-chain stage are 128 bytes");

enum : uint32_t { RCW_RING = 8 };   // beside BCW_TOP / BCW_HEAD / BCW_LAST in the same word
static_assert((RCW_RING & (BCW_TOP | BCW_HEAD | BCW_LAST)) == 0, "the ring bit is a bit of its own");

// rounds of the election: the least k with 2^k >= n_top, and one more
inline uint32_t ring_rounds(uint64_t n_top) {
    uint32_t k = 0;
    while ((1ull << k) < n_top) ++k;
    return k + 1;
}

__global__ __launch_bounds__(256) void k_rc_init(uint32_t n_order, const uint32_t* __restrict__ jb, uint32_t* __restrict__ ptr,
                                                 uint32_t* __restrict__ mn) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        const uint32_t j = jb[r];
        ptr[r] = j < n_order ? j : r;   // (cannot be out of range: k_bc_heads wrote pred or r)
        mn[r] = r;
    }
}

__global__ __launch_bounds__(256) void k_rc_round(uint32_t n_order, const uint32_t* __restrict__ ptr_in, const uint32_t* __restrict__ mn_in,
                                                  uint32_t* __restrict__ ptr_out, uint32_t* __restrict__ mn_out) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        const uint32_t p = ptr_in[r], m = mn_in[r];
        if (p >= n_order) {   // (cannot happen: ptr starts in range and only takes values of ptr)
            ptr_out[r] = r;
            mn_out[r] = m;
            continue;
        }
        const uint32_t mp = mn_in[p];
        ptr_out[r] = ptr_in[p];
        mn_out[r] = mp < m ? mp : m;
    }
}

__global__ __launch_bounds__(256) void k_rc_leaders(uint32_t n_order, const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ mn,
                                                    uint32_t* fw, uint32_t* __restrict__ jb, uint32_t* __restrict__ hops,
                                                    unsigned long long* __restrict__ counters) {
    uint64_t c[1] = {0};
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        if (mn[r] != r) continue;
        const uint32_t x = fw[r], p = ptr[r];
        if (!(x & BCW_TOP) || (x & BCW_HEAD) || p >= n_order) continue;
        // (p lies on r's own path or ring; on a ring no other thread writes its word: r is the ring's one leader)
        if (fw[p] & BCW_HEAD) continue;   // the head of r's path
        fw[r] = x | BCW_HEAD | RCW_RING;
        jb[r] = r;
        hops[r] = 0;
        ++c[0];
    }
    const uint64_t s = wave_sum64(c[0]);
    if (lane_id() == 0 && s) {
        atomicAdd(&counters[HK_HEADS], (unsigned long long)s);
        atomicAdd(&counters[HKR_RINGS], (unsigned long long)s);
    }
}

__global__ __launch_bounds__(256) void k_rc_close(uint32_t n_order, const uint32_t* __restrict__ fw, const uint32_t* __restrict__ cb,
                                                  uint32_t* __restrict__ last, unsigned long long* __restrict__ counters) {
    uint64_t c[1] = {0};
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_order; r += gridDim.x * blockDim.x) {
        if (!(fw[r] & RCW_RING)) continue;
        last[r] = r;
        c[0] += cb[r];
    }
    const uint64_t s = wave_sum64(c[0]);
    if (lane_id() == 0 && s) atomicAdd(&counters[HKR_RBUBBLES], (unsigned long long)s);
}

}  // namespace po
