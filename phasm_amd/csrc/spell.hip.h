// Device side of spelling: the DNA of graph paths out of the reads that are resident in HBM -- what
//   AssemblyGraph.sequence_for_path       phasm/assembly_graph.py:67-87
//   SequenceSource.get_sequence           phasm/io/sequences.py:32-65
// return, once the host has reduced every path to PIECES (phasm_amd/spelling.py): piece p = (oriented read, take) stands for the
// first `take` bytes of that read, 0 <= take <= its length, and a sequence is the concatenation of its pieces with ASCII a-z
// as A-Z and every other byte as it was added.
//   k_spell_offsets  the 32-bit scan of the takes (the library's prefix_sum; the host has checked that the total is below
//                    2^32) as 64-bit piece offsets, and the offsets at the sequence boundaries
//   k_spell_decode   one lane = 16 consecutive output bytes = one 16-byte store.  The lane finds the piece that holds its first
//                    byte by binary search over the piece offsets, then walks on through the pieces -- takes of 0 and 1 exist,
//                    a chunk may cover many -- until its 16 bytes are full or the pieces end.  bits == 2: 32 bits of codes out
//                    of one or two adjacent words of the read (base i at bits [2i, 2i + 2)), turned into letters by arithmetic
//                    on four bytes at a time.  bits == 8: the bytes out of at most three words, upper-cased in the word.  A word
//                    is loaded only where the piece has a byte in it, so every load lies inside the read.
//   k_spell_patch    (2-bit store with exception records) per piece the records of its read with pos < take, found by binary
//                    search in the read's ascending exc_pos segment: upper(exc_byte) at piece offset + pos.  Runs after the
//                    decode on the same stream; pieces do not overlap in the output, so no byte has two writers.
// The kernels read the device store as it is: an odd read's words are whatever the upload put there (copied, or rebuilt by
// k_revcomp_store); nothing is complemented here.
// `first_byte` (a multiple of 16) and `n_out` describe the window of the output that `out` holds: the library passes 0 and the
// padded total; the host emulation (tools/spell_host_emu.cpp) passes a window far into a long output, so that the 64-bit
// arithmetic runs.  No atomics, no LDS; every loop is bounded by a count.
#pragma once

namespace po {

struct alignas(16) SpellChunk {   // 16 output bytes, written with one store
    uint64_t lo, hi;
};

// four 2-bit codes (the low byte of x) as four letters, byte k = code k: 'A' + 2 * bit0 + 6 * bit1 + 11 * (bit0 & bit1) gives
// A C G T = 0x41 0x43 0x47 0x54; no byte carries into its neighbour
__device__ inline uint32_t spell_letters4(uint32_t x) {
    uint32_t t = (x | (x << 12)) & 0x000F000Fu;
    t = (t | (t << 6)) & 0x03030303u;
    const uint32_t b0 = t & 0x01010101u, b1 = (t >> 1) & 0x01010101u;
    return 0x41414141u + (b0 << 1) + b1 * 6u + (b0 & b1) * 11u;
}

// sixteen codes as sixteen letters
__device__ inline SpellChunk spell_letters16(uint32_t codes) {
    SpellChunk c;
    c.lo = (uint64_t)spell_letters4(codes & 0xFFu) | ((uint64_t)spell_letters4((codes >> 8) & 0xFFu) << 32);
    c.hi = (uint64_t)spell_letters4((codes >> 16) & 0xFFu) | ((uint64_t)spell_letters4(codes >> 24) << 32);
    return c;
}

// a-z as A-Z in all eight bytes of a word at once; bytes >= 0x80 stay
__device__ inline uint64_t spell_upper8(uint64_t x) {
    const uint64_t hept = x & 0x7F7F7F7F7F7F7F7Full;
    const uint64_t ge_a = hept + 0x1F1F1F1F1F1F1F1Full;   // bit 7 of a byte: its low seven bits >= 'a'
    const uint64_t gt_z = hept + 0x0505050505050505ull;   // ... > 'z'
    const uint64_t lower = ge_a & ~gt_z & ~x & 0x8080808080808080ull;
    return x ^ (lower >> 2);
}

__device__ inline uint8_t spell_upper(uint8_t b) { return (b >= (uint8_t)'a' && b <= (uint8_t)'z') ? (uint8_t)(b - 32u) : b; }

// bytes [skip, skip + n) of a read, 1 <= n <= 16, in the low n bytes of the chunk (the bytes above are not defined)
template <int BITS>
__device__ inline SpellChunk spell_fetch(const uint64_t* __restrict__ w, uint32_t skip, uint32_t n) {
    if (BITS == 2) {
        const uint32_t i = skip >> 5, sh = (skip & 31u) * 2u;
        uint64_t codes = w[i] >> sh;
        if ((skip & 31u) + n > 32u) codes |= w[i + 1] << (64u - sh);   // (sh > 0 here)
        return spell_letters16((uint32_t)codes);
    }
    const uint32_t i = skip >> 3, b = skip & 7u, sh = b * 8u;
    const uint64_t w0 = w[i], w1 = b + n > 8u ? w[i + 1] : 0ull, w2 = b + n > 16u ? w[i + 2] : 0ull;
    SpellChunk c;
    c.lo = sh ? (w0 >> sh) | (w1 << (64u - sh)) : w0;
    c.hi = sh ? (w1 >> sh) | (w2 << (64u - sh)) : w1;
    c.lo = spell_upper8(c.lo);
    c.hi = spell_upper8(c.hi);
    return c;
}

// the low n bytes of `c` (1 <= n <= 16) into bytes [at, at + n) of `acc`, at + n <= 16; the bytes of acc from `at` up are zero
__device__ inline void spell_place(SpellChunk& acc, SpellChunk c, uint32_t at, uint32_t n) {
    if (n < 8u) {
        c.lo &= (1ull << (8u * n)) - 1ull;
        c.hi = 0;
    } else if (n < 16u) {
        c.hi &= n == 8u ? 0ull : (1ull << (8u * (n - 8u))) - 1ull;
    }
    if (at >= 8u) {
        acc.hi |= c.lo << (8u * (at - 8u));
    } else if (at) {
        acc.hi |= (c.hi << (8u * at)) | (c.lo >> (64u - 8u * at));
        acc.lo |= c.lo << (8u * at);
    } else {
        acc.lo |= c.lo;
        acc.hi |= c.hi;
    }
}

// scan[i] (exclusive, scan[n_pieces] the total; nullptr when there is no piece: every offset is 0) -> piece_off[n_pieces + 1]
// and seq_byte_off[n_seqs + 1]
__global__ __launch_bounds__(256) void k_spell_offsets(const uint32_t* __restrict__ scan, uint32_t n_pieces, const uint64_t* __restrict__ seq_off,
                                                       uint32_t n_seqs, uint64_t* __restrict__ piece_off, uint64_t* __restrict__ seq_byte_off) {
    const uint32_t n = (n_pieces > n_seqs ? n_pieces : n_seqs) + 1u;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        if (i <= n_pieces) piece_off[i] = scan ? scan[i] : 0u;
        if (i <= n_seqs) {
            const uint64_t p = seq_off[i];
            seq_byte_off[i] = scan && p <= n_pieces ? scan[p] : 0u;
        }
    }
}

// (bits: 2 or 8, the encoding of the store -- the same for every lane of a launch)
__global__ __launch_bounds__(256) void k_spell_decode(const uint64_t* __restrict__ words, const uint64_t* __restrict__ woff, uint32_t bits,
                                                      const uint32_t* __restrict__ piece_read, const uint32_t* __restrict__ piece_take,
                                                      const uint64_t* __restrict__ piece_off, uint32_t n_pieces, uint64_t first_byte,
                                                      uint64_t n_chunks, SpellChunk* __restrict__ out) {
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_chunks; c += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t b0 = first_byte + c * 16u;
        // the last piece that begins at or before b0: pieces of take 0 before it share its offset and hold nothing
        uint32_t lo = 0, hi = n_pieces;
        while (lo < hi) {   // the first p in [0, n_pieces] with piece_off[p] > b0 (piece_off[0] = 0: it is at least 1)
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (piece_off[mid] > b0) hi = mid; else lo = mid + 1;
        }
        uint32_t p = lo ? lo - 1 : 0;
        SpellChunk acc = {0, 0};
        uint32_t filled = 0;
        while (filled < 16u && p < n_pieces) {
            const uint64_t at = b0 + filled, off = piece_off[p];
            const uint32_t take = piece_take[p];
            if (at < off || at - off >= take) {   // (an empty piece, or one that ends before this chunk)
                ++p;
                continue;
            }
            const uint32_t skip = (uint32_t)(at - off), n = take - skip < 16u - filled ? take - skip : 16u - filled;
            const uint64_t* w = words + woff[piece_read[p]];
            spell_place(acc, bits == 2u ? spell_fetch<2>(w, skip, n) : spell_fetch<8>(w, skip, n), filled, n);
            filled += n;
            if (skip + n == take) ++p;
        }
        out[c] = acc;
    }
}

__global__ __launch_bounds__(256) void k_spell_patch(const uint32_t* __restrict__ piece_read, const uint32_t* __restrict__ piece_take,
                                                     const uint64_t* __restrict__ piece_off, uint32_t n_pieces,
                                                     const uint32_t* __restrict__ exc_off, const uint32_t* __restrict__ exc_pos,
                                                     const uint8_t* __restrict__ exc_byte, uint64_t first_byte, uint64_t n_out,
                                                     uint8_t* __restrict__ out) {
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n_pieces; p += gridDim.x * blockDim.x) {
        const uint32_t r = piece_read[p], take = piece_take[p], e0 = exc_off[r], e1 = exc_off[r + 1];
        if (e0 == e1 || !take) continue;
        uint32_t lo = e0, hi = e1;   // the first record of the read with pos >= take
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (exc_pos[mid] < take) lo = mid + 1; else hi = mid;
        }
        const uint64_t off = piece_off[p];
        for (uint32_t e = e0; e < lo; ++e) {
            const uint64_t at = off + exc_pos[e];
            if (at >= first_byte && at - first_byte < n_out) out[at - first_byte] = spell_upper(exc_byte[e]);
        }
    }
}

}  // namespace po
