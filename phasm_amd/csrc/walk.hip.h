// Device side of the walk of `phasm phase` along a bubble chain: the candidate sets of
// BubbleChainPhaser (phasm/phasing.py:125-142, 311-319, 343-364) stay in HBM from bubble to bubble.
//
// Reads carry BLOCK-STABLE ids: the order in which they joined the block (the host numbers them, one merge per step).  The
// state is one bitset over those ids per (candidate, haplotype slot), rows of W = ceil(block reads / 32) words, the log_rl of
// every candidate, and per advanced bubble the (parent, extension) of every candidate that survived it.  A step scores through
// the kernels of phase.hip.h, whose k_ph_intervals reads the state's rows; what is new here is what carries the state on:
//   k_wk_advance   one thread per (new slot, word): the parent's row | the path's row, into the OTHER half of a ping-pong
//                  pair whose rows have the new length (every word of every new row is written: nothing stale can stay);
//                  the thread of word 0 of slot 0 also notes the candidate's (parent, extension) and its log_rl
//   k_wk_trace     one thread per named candidate: back through the links of every depth, its extension id at each
//   k_wk_max       the greatest log_rl, by the order-keeping key and integer atomicMax of k_ph_gather
//   k_wk_pick      the candidates whose keep byte is set (k_ph_survive at level 0 wrote it) to their places (the library's
//                  prefix sum): the tie set of prune(.., 1.0), ascending
// Integer atomics only.  Memory: 4 W per slot twice, 8 per candidate twice, 8 per survivor of every advanced bubble.
#pragma once

namespace po {

struct WkLink {
    uint32_t parent, ext;   // the candidate of the bubble before that this one extends, and by which extension id
};

__global__ __launch_bounds__(256) void k_wk_advance(uint32_t n_new, uint32_t n_old, uint32_t k, uint32_t P, uint32_t W_old, uint32_t W_new,
                                                    const uint32_t* __restrict__ old_rows, const uint32_t* __restrict__ path_rows,
                                                    const uint32_t* __restrict__ cand, const uint32_t* __restrict__ ext,
                                                    const double* __restrict__ rl, uint32_t* __restrict__ new_rows,
                                                    WkLink* __restrict__ links, double* __restrict__ new_rl) {
    const unsigned long long total = (unsigned long long)n_new * k * W_new;
    for (unsigned long long x = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (unsigned long long)gridDim.x * blockDim.x) {
        const uint32_t w = (uint32_t)(x % W_new);
        const unsigned long long slot = x / W_new;
        const uint32_t j = (uint32_t)(slot / k), i = (uint32_t)(slot % k);
        const uint32_t c = cand[j];
        uint32_t e = ext[j];
        for (uint32_t t = k - 1; t > i; --t) e /= P;   // digits base P, slot 0 most significant
        uint32_t v = path_rows[(size_t)(e % P) * W_new + w];
        if (w < W_old && c < n_old) v |= old_rows[((size_t)c * k + i) * W_old + w];
        new_rows[x] = v;
        if (w == 0 && i == 0) {
            links[j] = WkLink{c, ext[j]};
            new_rl[j] = rl[j];
        }
    }
}

// level_off[d] .. level_off[d + 1]: the links of the candidates that survived the d-th advanced bubble of the block
__global__ __launch_bounds__(256) void k_wk_trace(uint32_t n, uint32_t depth, const unsigned long long* __restrict__ level_off,
                                                  const WkLink* __restrict__ links, const uint32_t* __restrict__ cands,
                                                  uint32_t* __restrict__ ext_out) {
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < n; q += gridDim.x * blockDim.x) {
        uint32_t c = cands[q];
        for (uint32_t d = depth; d-- > 0;) {
            const unsigned long long lo = level_off[d], hi = level_off[d + 1];
            if (c >= hi - lo) {   // (cannot happen: the host refused a candidate past the list, a parent is a place of the level before)
                ext_out[(size_t)q * depth + d] = 0xFFFFFFFFu;
                continue;
            }
            const WkLink l = links[lo + c];
            ext_out[(size_t)q * depth + d] = l.ext;
            c = l.parent;
        }
    }
}

__global__ __launch_bounds__(256) void k_wk_max(uint32_t n, const double* __restrict__ rl, unsigned long long* __restrict__ max_key) {
    unsigned long long best = 0;
    for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n; x += gridDim.x * blockDim.x) {
        const double v = rl[x];
        if (v != v) continue;   // (a NaN is never kept, so none is here)
        const unsigned long long key = ph_key(v);
        best = key > best ? key : best;
    }
    for (int o = 1; o < WAVE; o <<= 1) {
        const unsigned long long other = __shfl_xor(best, o, WAVE);
        best = other > best ? other : best;
    }
    if (lane_id() == 0 && best) atomicMax(max_key, best);
}

__global__ __launch_bounds__(256) void k_wk_pick(uint32_t n, uint32_t n_out, const uint8_t* __restrict__ keep, const uint32_t* __restrict__ place,
                                                 uint32_t* __restrict__ out) {
    for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n; x += gridDim.x * blockDim.x) {
        if (!keep[x]) continue;
        const uint32_t at = place[x];
        if (at < n_out) out[at] = x;   // (always: the prefix sum counted this entry)
    }
}

}  // namespace po
