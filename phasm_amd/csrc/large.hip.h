// Device side of the large-bubble arm of `phasm phase`: what phase_large_bubble computes
//   phasm/phasing.py:633-685
// for a bubble whose paths po_phase_paths left listed in HBM -- the score of EVERY listed path against the relevant reads and
// the n_best best of them -- without the 64-path limit of po_phase_branch and without a path leaving the device.
//
// The score of a path is the sum over the relevant reads r of f(r; interior reads of the path) / R, with f as in phase.hip.h:
// (E - S0) / overlap_max_r if S0 < E else 0, S0 the least arange[0] and E the greatest min(overlap_max_r, arange[1]) over the
// alignments of r whose b read lies on the path.  Least and greatest of a union are the least and greatest of the parts, so
// an interval (S0, E) per (interior NODE, read) suffices: k_ph_bits and k_ph_intervals compute it with the bubble's interior
// nodes as their "sets", and a path joins the intervals of its nodes with min and max.
//   k_lg_slots     node id -> interior slot of the bubble (the map is set to LG_NO_SLOT by a memset before; entrance, exit and
//                  every node outside the bubble keep that value)
//   k_lg_score     one workgroup per path, grid-stride: the path's slots staged in LDS LG_CHUNK at a time, the reads in tiles of
//                  PH_TILE; per read the join over the path's slots (the partial join of a tile's reads waits in LDS between
//                  chunks, every thread touching its own reads alone), then the sum in EXACTLY the order of k_ph_table -- every
//                  thread its reads in index order, the wave by ph_wave_sum, thread 0 the waves in wave order and the tiles in
//                  tile order -- so the sum has the bits of S[0][0][p] of po_phase_branch with an empty read set; then
//                  score = sum / R on the device (the reference ranks the quotients)
//   k_lg_best_key  round j of the selection: the greatest ph_key(score) among the paths not picked in rounds 0..j-1
//   k_lg_best_idx  the least index among those paths whose key is that greatest one: entry j of the result
// The stable descending sort of the reference puts the lower index first among equal scores; that is what the two kernels do
// per round.  Integer atomics only (atomicMax on the key, atomicMin on the index), no floating-point atomics.
// Memory beyond the inputs: 8 bytes per (interior node, read), 4 W per interior node, 4 per node of the graph (the slot map),
// 8 per listed path of the bubble (the scores).  Static LDS of k_lg_score: 2 x 4 x PH_TILE + 4 x LG_CHUNK + 8 x 4 bytes = 17 KB.
#pragma once

namespace po {

constexpr uint32_t LG_CHUNK = 256;              // interior slots of a path staged in LDS at a time (one per thread)
constexpr uint32_t LG_MAX_BEST = 8;
constexpr uint32_t LG_NO_SLOT = 0xFFFFFFFFu;
constexpr unsigned long long LG_NO_INDEX = 0xFFFFFFFFFFFFFFFFull;

// counters of a call: the longest path seen; then LG_MAX_BEST keys and LG_MAX_BEST indices
enum { LK_MAXLEN = 0, LK_KEY = 1, LK_BEST = LK_KEY + LG_MAX_BEST, LK_N = LK_BEST + LG_MAX_BEST };

__global__ __launch_bounds__(256) void k_lg_slots(uint32_t n_inside, const uint32_t* __restrict__ inside_nodes, uint32_t n_total,
                                                  uint32_t* __restrict__ slot_of) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_inside; i += gridDim.x * blockDim.x) {
        const uint32_t node = inside_nodes[i];
        if (node < n_total) slot_of[node] = i;   // (a node is interior to one top-level bubble and listed there once)
    }
}

__global__ __launch_bounds__(256) void k_lg_score(uint32_t P, uint32_t R, uint32_t n_inside, uint32_t n_total, const uint32_t* __restrict__ path_off,
                                                  const uint32_t* __restrict__ path_nodes, const uint32_t* __restrict__ slot_of,
                                                  const PhInterval* __restrict__ node_iv, const int32_t* __restrict__ omax,
                                                  double* __restrict__ score, unsigned long long* __restrict__ cnt) {
    __shared__ int32_t s_s0[PH_TILE], s_e[PH_TILE];
    __shared__ uint32_t s_slot[LG_CHUNK];
    __shared__ double s_part[256 / WAVE];
    for (uint32_t p = blockIdx.x; p < P; p += gridDim.x) {
        const uint32_t lo = path_off[p], hi = path_off[p + 1];   // (path_off points at the bubble's first listed path)
        const uint32_t len = hi > lo ? hi - lo : 0u;
        double total = 0.0;
        for (uint32_t base = 0; base < R; base += PH_TILE) {
            const uint32_t n = R - base < PH_TILE ? R - base : PH_TILE;
            for (uint32_t t = threadIdx.x; t < n; t += blockDim.x) {
                s_s0[t] = PH_NO_START;
                s_e[t] = 0;
            }
            for (uint32_t c0 = 0; c0 < len; c0 += LG_CHUNK) {
                const uint32_t m = len - c0 < LG_CHUNK ? len - c0 : LG_CHUNK;
                __syncthreads();   // (the chunk before is read no more)
                for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) {
                    const uint32_t node = path_nodes[(size_t)lo + c0 + i];
                    const uint32_t slot = node < n_total ? slot_of[node] : LG_NO_SLOT;
                    s_slot[i] = slot < n_inside ? slot : LG_NO_SLOT;   // (entrance and exit: none)
                }
                __syncthreads();
                for (uint32_t t = threadIdx.x; t < n; t += blockDim.x) {
                    int32_t s0 = s_s0[t], e = s_e[t];
                    for (uint32_t i = 0; i < m; ++i) {
                        const uint32_t slot = s_slot[i];   // (the same for every thread: no divergence)
                        if (slot == LG_NO_SLOT) continue;
                        const PhInterval v = node_iv[(unsigned long long)slot * R + base + t];
                        s0 = v.s0 < s0 ? v.s0 : s0;
                        e = v.e > e ? v.e : e;
                    }
                    s_s0[t] = s0;
                    s_e[t] = e;
                }
            }
            double acc = 0.0;
            for (uint32_t t = threadIdx.x; t < n; t += blockDim.x) {
                const int32_t s0 = s_s0[t], e = s_e[t];
                if (s0 < e) acc += (double)((long long)e - (long long)s0) / (double)omax[base + t];
            }
            acc = ph_wave_sum(acc);
            if (lane_id() == 0) s_part[threadIdx.x / WAVE] = acc;
            __syncthreads();
            if (threadIdx.x == 0) {
                double sum = 0.0;
                for (uint32_t w = 0; w < blockDim.x / WAVE; ++w) sum += s_part[w];
                total = base ? total + sum : sum;   // (the tiles in tile order, as k_ph_table adds them)
            }
            __syncthreads();   // (s_part and the tile's joins are read no more)
        }
        if (threadIdx.x == 0) {
            score[p] = total / (double)R;
            atomicMax(cnt + LK_MAXLEN, (unsigned long long)len);
        }
    }
}

// whether path p was picked in one of the rounds before `round`
__device__ inline bool lg_taken(const unsigned long long* best, uint32_t round, uint32_t p) {
    bool taken = false;
    for (uint32_t j = 0; j < round && j < LG_MAX_BEST; ++j) taken = taken || best[j] == p;
    return taken;
}

__global__ __launch_bounds__(256) void k_lg_best_key(uint32_t P, uint32_t round, const double* __restrict__ score, unsigned long long* __restrict__ cnt) {
    unsigned long long mine = 0;   // (below every key)
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) {
        if (lg_taken(cnt + LK_BEST, round, p)) continue;
        const unsigned long long key = ph_key(score[p]);
        mine = key > mine ? key : mine;
    }
    if (mine) atomicMax(cnt + LK_KEY + round, mine);
}

__global__ __launch_bounds__(256) void k_lg_best_idx(uint32_t P, uint32_t round, const double* __restrict__ score, unsigned long long* __restrict__ cnt) {
    const unsigned long long top = cnt[LK_KEY + round];
    unsigned long long mine = LG_NO_INDEX;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) {
        if (ph_key(score[p]) != top || lg_taken(cnt + LK_BEST, round, p)) continue;
        mine = p < mine ? p : mine;
    }
    if (mine != LG_NO_INDEX) atomicMin(cnt + LK_BEST + round, mine);
}

}   // namespace po
