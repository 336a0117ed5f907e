// Device side of the RESIDENT route through one step of the walk of `phasm phase`: the gather of
// po_walk_relevant stays in buffers of the walk, and what run_walk_step does on the host between the gather and the scoring --
// numbering the reads of b_reads that are new to the block, rewriting aln_b and the path ids to block-stable ids, keeping the
// map -- happens here.  The map is one array over the handle's read ids, stable_of[global id] (RS_NONE: not in the block), and
// its inverse global_of[stable id]; prev_graph and prev_aligning are two bitsets over the read ids.
//   k_rs_flag      one thread per read of b_reads: 1 where the read is new to the block
//   k_rs_local     after the library's prefix sum over the flags: local id -> stable id (a known read keeps its id, the new
//                  ones get n_block + their rank among the new ones, in the order of b_reads)
//   k_rs_alnb      aln_b through that translation
//   k_rs_paths     the path ids, global -> local (a rank query on the words of G) -> stable; a read outside G becomes RS_NONE,
//                  which k_ph_bits ignores (it is not below n_b)
//   k_rs_commit    after a step that advanced: the new ids into stable_of, the new reads behind global_of
//   k_rs_or        after a step that advanced: prev_graph |= cur_graph, prev_aligning |= cur_aligning, word by word
//   k_rs_unmap     the lazy half of po_walk_reset: stable_of back to RS_NONE over global_of[0 .. n_block)
//   k_rs_popc      the set bits of every word (po_walk_prev_copy lists a set through the library's prefix sum and k_rr_list)
// Integer only, no atomics: every thread writes places of its own (b_reads is strictly ascending, stable ids are distinct).
#pragma once

namespace po {

constexpr uint32_t RS_NONE = 0xFFFFFFFFu;

__global__ __launch_bounds__(256) void k_rs_flag(uint32_t n_b, const uint32_t* __restrict__ b_reads, uint32_t n_ids,
                                                 const uint32_t* __restrict__ stable_of, uint32_t* __restrict__ flag) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n_b; j += gridDim.x * blockDim.x) {
        const uint32_t g = b_reads[j];
        flag[j] = g < n_ids && stable_of[g] == RS_NONE;   // (the gather lists only ids below n_ids)
    }
}

__global__ __launch_bounds__(256) void k_rs_local(uint32_t n_b, const uint32_t* __restrict__ b_reads, uint32_t n_ids,
                                                  const uint32_t* __restrict__ stable_of, uint32_t n_block,
                                                  const uint32_t* __restrict__ flag, const uint32_t* __restrict__ rank,
                                                  uint32_t* __restrict__ xl) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n_b; j += gridDim.x * blockDim.x) {
        const uint32_t g = b_reads[j];
        xl[j] = flag[j] ? n_block + rank[j] : (g < n_ids ? stable_of[g] : RS_NONE);
    }
}

__global__ __launch_bounds__(256) void k_rs_alnb(uint32_t n_aln, const uint32_t* __restrict__ aln_b, uint32_t n_b,
                                                 const uint32_t* __restrict__ xl, uint32_t* __restrict__ out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_aln; i += gridDim.x * blockDim.x) {
        const uint32_t b = aln_b[i];
        out[i] = b < n_b ? xl[b] : RS_NONE;
    }
}

// g_bits / g_rank: the words of G and the number of its reads in the words before (the ranks the gather listed b_reads by)
__global__ __launch_bounds__(256) void k_rs_paths(uint32_t n, const uint32_t* __restrict__ ids, uint32_t n_ids,
                                                  const uint32_t* __restrict__ g_bits, const uint32_t* __restrict__ g_rank, uint32_t n_b,
                                                  const uint32_t* __restrict__ xl, uint32_t* __restrict__ out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t g = ids[i];
        uint32_t v = RS_NONE;
        if (g < n_ids) {
            const uint32_t word = g_bits[g >> 5];
            if ((word >> (g & 31)) & 1u) {
                const uint32_t local = g_rank[g >> 5] + (uint32_t)__popc(word & ((1u << (g & 31)) - 1u));
                if (local < n_b) v = xl[local];
            }
        }
        out[i] = v;
    }
}

__global__ __launch_bounds__(256) void k_rs_commit(uint32_t n_b, const uint32_t* __restrict__ b_reads, uint32_t n_ids,
                                                   const uint32_t* __restrict__ flag, const uint32_t* __restrict__ xl, uint32_t n_after,
                                                   uint32_t* __restrict__ stable_of, uint32_t* __restrict__ global_of) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n_b; j += gridDim.x * blockDim.x) {
        if (!flag[j]) continue;
        const uint32_t g = b_reads[j], s = xl[j];
        if (g >= n_ids || s >= n_after) continue;   // (cannot happen: the flag says g < n_ids, the host sized global_of by the count)
        stable_of[g] = s;
        global_of[s] = g;
    }
}

__global__ __launch_bounds__(256) void k_rs_or(uint32_t W, const uint32_t* __restrict__ cur_graph, const uint32_t* __restrict__ cur_aligning,
                                               uint32_t* __restrict__ prev_graph, uint32_t* __restrict__ prev_aligning) {
    for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < W; w += gridDim.x * blockDim.x) {
        prev_graph[w] |= cur_graph[w];
        prev_aligning[w] |= cur_aligning[w];
    }
}

__global__ __launch_bounds__(256) void k_rs_unmap(uint32_t n, const uint32_t* __restrict__ global_of, uint32_t n_ids,
                                                  uint32_t* __restrict__ stable_of) {
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
        const uint32_t g = global_of[s];
        if (g < n_ids) stable_of[g] = RS_NONE;
    }
}

__global__ __launch_bounds__(256) void k_rs_popc(uint32_t W, const uint32_t* __restrict__ bits, uint32_t* __restrict__ cnt) {
    for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < W; w += gridDim.x * blockDim.x) cnt[w] = (uint32_t)__popc(bits[w]);
}

}  // namespace po
