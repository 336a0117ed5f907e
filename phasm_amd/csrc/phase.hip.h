// Device side of the hot loop of `phasm phase`: what BubbleChainPhaser.branch computes at one bubble,
//   generate_new_hsets + calculate_rl   phasm/phasing.py:421-480, 564-631
//   prune                               phasm/phasing.py:482-539
// and the per-path score of phase_large_bubble (phasing.py:633-685), on one bubble given as plain arrays of LOCAL read ids
// (0 .. n_b-1: the graph reads that occur as b read of an alignment of a relevant read).
//
// The reference walks every relevant read and every alignment once per (candidate set, k-tuple of paths).  That loop
// decomposes: the overlap of read r with the reads of haplotype slot i of candidate c extended by path p depends on
// (c, i, p) alone, so
//   S[c][i][p] = sum over the relevant reads r of f(r; reads(c, i) + interior(p)),   f = (E - S0) / overlap_max_r if S0 < E else 0
// with S0 the least arange[0] and E the greatest min(overlap_max_r, arange[1]) (never below 0) of the alignments of r whose b
// read is in the set.  Least and greatest of a union are the least and greatest of the parts, so (S0, E) is kept per (read set,
// read) and per (path, read) and joined in the table kernel.
//   k_ph_bits        one thread per read set or path: its local ids into a bitset of W = ceil(n_b / 32) words (cleared by a
//                    memset before; one writer per set, no atomics)
//   k_ph_intervals   one thread per (set or path, read): (S0, E) over the read's alignments whose b read has its bit set
//   k_ph_table       one workgroup per slot (c, i), grid-stride: the slot's intervals and the reads' overlap_max in LDS, tile
//                    by tile of PH_TILE reads; per path the sum over the tile's reads -- every thread adds its reads in
//                    index order, the wave adds by a butterfly, thread 0 adds the waves in wave order and the tiles in tile
//                    order: a fixed order, float64, the same bits on every run
//   k_ph_extend      one thread per (candidate, extension id), a workgroup takes one chunk of one candidate per step, that
//                    candidate's k x P slice of S in LDS: digits base P (slot 0 most significant), the start-of-block test
//                    (non-decreasing digits), the sum in slot order, the multinomial from the multiplicities, rl, the keep byte
//   k_ph_gather      the entries whose byte is set to their places (the library's prefix sum over the bytes), in id order =
//                    (candidate, extension) order; the greatest rl of them through an integer atomicMax on an order-keeping key
//   k_ph_levels      per kept entry the number of prune levels it survives (the levels as running maxima, so a binary search),
//                    counted per workgroup in LDS and added to the histogram with integer atomics
//   k_ph_survive     the keep byte of the level the host picked
// No kernel passes over reads per extension.  Integer atomics only; no floating-point atomics anywhere.
// Memory: 8 bytes per (set or path, read), 4 W per set or path, 8 per table entry, 13 per extension id (rl, byte, place), all
// allocated before the first launch; 21 per kept entry (the entry, byte, place) and 16 per survivor once their numbers are known.
#pragma once

namespace po {

constexpr uint32_t PH_TILE = 2048;         // reads per LDS tile of k_ph_table: 3 x 4 bytes each, 24 KB
constexpr uint32_t PH_MAX_K = 8, PH_MAX_P = 64;
constexpr uint32_t PH_MAX_LEVELS = 1024;   // prune levels of one call (the LDS histogram of k_ph_levels)
constexpr int32_t PH_NO_START = 0x7FFFFFFF;

enum { PK_ENUM = 0, PK_KEPT = 1, PK_N = 2 };

struct PhInterval {
    int32_t s0, e;   // least arange[0] (PH_NO_START: no alignment matched), greatest min(overlap_max, arange[1]) or 0
};

// a double as a 64-bit key whose unsigned order is the order of the doubles (no NaN goes in); 0 is below every key
__device__ inline unsigned long long ph_key(double v) {
    unsigned long long b;
    memcpy(&b, &v, 8);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ inline double ph_wave_sum(double v) {
    for (int o = 1; o < WAVE; o <<= 1) v += __shfl_xor(v, o, WAVE);   // (a + b == b + a bit for bit: every lane holds the same sum)
    return v;
}

__global__ __launch_bounds__(256) void k_ph_bits(uint32_t n_sets, const uint32_t* __restrict__ off, const uint32_t* __restrict__ ids,
                                                 uint32_t n_b, uint32_t W, uint32_t* __restrict__ bits) {
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < n_sets; s += gridDim.x * blockDim.x) {
        uint32_t* mine = bits + (size_t)s * W;
        for (uint32_t j = off[s]; j < off[s + 1]; ++j) {
            const uint32_t id = ids[j];
            if (id < n_b) mine[id >> 5] |= 1u << (id & 31);   // (the host refused ids at or above n_b)
        }
    }
}

__global__ __launch_bounds__(256) void k_ph_intervals(uint32_t n_sets, uint32_t R, uint32_t n_b, uint32_t W, const uint32_t* __restrict__ bits,
                                                      const uint32_t* __restrict__ aln_off, const uint32_t* __restrict__ aln_b,
                                                      const int32_t* __restrict__ a0, const int32_t* __restrict__ a1,
                                                      const int32_t* __restrict__ omax, PhInterval* __restrict__ iv) {
    const unsigned long long total = (unsigned long long)n_sets * R;
    for (unsigned long long x = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (unsigned long long)gridDim.x * blockDim.x) {
        const uint32_t s = (uint32_t)(x / R), r = (uint32_t)(x % R);
        const uint32_t* mine = bits + (size_t)s * W;
        const int32_t om = omax[r];
        int32_t s0 = PH_NO_START, e = 0;
        for (uint32_t j = aln_off[r]; j < aln_off[r + 1]; ++j) {
            const uint32_t b = aln_b[j];
            if (b >= n_b || !((mine[b >> 5] >> (b & 31)) & 1u)) continue;
            const int32_t lo = a0[j], hi = a1[j] < om ? a1[j] : om;
            s0 = lo < s0 ? lo : s0;
            e = hi > e ? hi : e;
        }
        iv[x] = PhInterval{s0, e};
    }
}

__global__ __launch_bounds__(256) void k_ph_table(uint32_t n_slots, uint32_t P, uint32_t R, const PhInterval* __restrict__ set_iv,
                                                  const PhInterval* __restrict__ path_iv, const int32_t* __restrict__ omax,
                                                  double* __restrict__ S) {
    __shared__ int32_t s_s0[PH_TILE], s_e[PH_TILE], s_om[PH_TILE];
    __shared__ double s_part[256 / WAVE];
    for (uint32_t slot = blockIdx.x; slot < n_slots; slot += gridDim.x) {
        for (uint32_t base = 0; base < R || base == 0; base += PH_TILE) {
            const uint32_t n = R - base < PH_TILE ? R - base : PH_TILE;
            __syncthreads();   // (the tile before is read no more)
            for (uint32_t t = threadIdx.x; t < n; t += blockDim.x) {
                const PhInterval v = set_iv[(size_t)slot * R + base + t];
                s_s0[t] = v.s0;
                s_e[t] = v.e;
                s_om[t] = omax[base + t];
            }
            __syncthreads();
            for (uint32_t p = 0; p < P; ++p) {
                double acc = 0.0;
                for (uint32_t t = threadIdx.x; t < n; t += blockDim.x) {
                    const PhInterval v = path_iv[(size_t)p * R + base + t];
                    const int32_t s0 = v.s0 < s_s0[t] ? v.s0 : s_s0[t], e = v.e > s_e[t] ? v.e : s_e[t];
                    if (s0 < e) acc += (double)((long long)e - (long long)s0) / (double)s_om[t];
                }
                acc = ph_wave_sum(acc);
                if (lane_id() == 0) s_part[threadIdx.x / WAVE] = acc;
                __syncthreads();
                if (threadIdx.x == 0) {
                    double sum = 0.0;
                    for (uint32_t w = 0; w < blockDim.x / WAVE; ++w) sum += s_part[w];
                    double* at = S + (size_t)slot * P + p;
                    *at = base ? *at + sum : sum;   // (one writer per entry: the tiles in tile order)
                }
                __syncthreads();
            }
            if (R == 0) break;
        }
    }
}

// Everything k_ph_extend needs beyond its arrays.  denom = k * R as a double (0: no relevant reads, every sum counts as 0);
// dead: fewer relevant reads than min_spanning_reads, every rl is -inf; log_thr = log10(threshold) or -inf.
struct PhExtend {
    uint32_t C, P, k, Pk, chunks, start_mode, dead, kfact;
    double denom, log_thr;
};

__global__ __launch_bounds__(256) void k_ph_extend(PhExtend a, const double* __restrict__ S, double* __restrict__ rl_out,
                                                   uint8_t* __restrict__ keep, unsigned long long* __restrict__ counters) {
    __shared__ double s_tab[PH_MAX_K * PH_MAX_P];
    uint64_t c[2] = {0, 0};   // enumerated, kept
    const uint32_t n_tiles = a.C * a.chunks, kP = a.k * a.P;
    uint32_t held = 0xFFFFFFFFu;
    const double ninf = -(double)INFINITY;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t cand = tile / a.chunks, chunk = tile % a.chunks;
        if (cand != held) {   // (uniform over the workgroup)
            __syncthreads();
            for (uint32_t t = threadIdx.x; t < kP; t += blockDim.x) s_tab[t] = S[(size_t)cand * kP + t];
            __syncthreads();
            held = cand;
        }
        const uint32_t ext = chunk * blockDim.x + threadIdx.x;
        if (ext >= a.Pk) continue;
        // digits base P, slot 0 most significant, six bits each
        unsigned long long digits = 0;
        uint32_t rest = ext;
        for (uint32_t i = a.k; i-- > 0;) {
            digits |= (unsigned long long)(rest % a.P) << (6 * i);
            rest /= a.P;
        }
        bool listed = true;
        double sum = 0.0;
        uint32_t den = 1;
#pragma unroll
        for (uint32_t i = 0; i < PH_MAX_K; ++i) {
            if (i >= a.k) break;
            const uint32_t d = (uint32_t)(digits >> (6 * i)) & 63u;
            if (i && d < ((uint32_t)(digits >> (6 * (i - 1))) & 63u)) listed = false;
            sum += s_tab[i * a.P + d];
            uint32_t same = 1;   // the slots up to this one with the same path
            for (uint32_t j = 0; j < i; ++j) same += (((uint32_t)(digits >> (6 * j)) & 63u) == d);
            den *= same;
        }
        const size_t id = (size_t)cand * a.Pk + ext;
        if (a.start_mode && !listed) {
            rl_out[id] = ninf;
            keep[id] = 0;
            continue;
        }
        double rl = ninf;
        if (!a.dead) {
            const double tot = a.denom > 0.0 ? sum / a.denom : 0.0;
            const double p_sr = tot == 0.0 ? ninf : log10(tot);
            const double prior = log10((double)(a.kfact / den) / (double)a.Pk);
            rl = p_sr + prior;
        }
        const bool kept = rl >= a.log_thr;
        rl_out[id] = rl;
        keep[id] = kept;
        ++c[0];
        c[1] += kept;
    }
    block_add<2>(c, counters + PK_ENUM);
}
static_assert(PK_KEPT == PK_ENUM + 1, "k_ph_extend adds the two in one go");
static_assert(PH_MAX_P <= 64 && PH_MAX_K * 6 <= 64, "a digit of k_ph_extend has six bits, eight of them share a word");

// The entries whose byte is set, to their places.  cand_in == NULL: entry x is extension id x (candidate x / Pk, extension
// x % Pk); else entry x of a list.  max_key (may be NULL): the greatest rl of the entries that went out.
__global__ __launch_bounds__(256) void k_ph_gather(uint32_t n, uint32_t n_out, uint32_t Pk, const uint8_t* __restrict__ keep,
                                                   const uint32_t* __restrict__ place, const uint32_t* __restrict__ cand_in,
                                                   const uint32_t* __restrict__ ext_in, const double* __restrict__ rl_in,
                                                   uint32_t* __restrict__ cand_out, uint32_t* __restrict__ ext_out, double* __restrict__ rl_out,
                                                   unsigned long long* __restrict__ max_key) {
    unsigned long long best = 0;
    for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n; x += gridDim.x * blockDim.x) {
        if (!keep[x]) continue;
        const uint32_t at = place[x];
        if (at >= n_out) continue;   // (cannot happen: the prefix sum counted this entry)
        const double rl = rl_in[x];
        cand_out[at] = cand_in ? cand_in[x] : x / Pk;
        ext_out[at] = ext_in ? ext_in[x] : x % Pk;
        rl_out[at] = rl;
        const unsigned long long key = ph_key(rl);
        best = key > best ? key : best;
    }
    if (!max_key) return;
    for (int o = 1; o < WAVE; o <<= 1) {
        const unsigned long long other = __shfl_xor(best, o, WAVE);
        best = other > best ? other : best;
    }
    if (lane_id() == 0 && best) atomicMax(max_key, best);
}

// the number of levels an entry at distance d = rl - max survives: levels[] are running maxima (non-decreasing), so the
// entries with levels[j] <= d are a prefix
__device__ inline uint32_t ph_survived(double d, const double* __restrict__ levels, uint32_t n_levels) {
    uint32_t lo = 0, hi = n_levels;   // levels[j] <= d for j < lo, not for j >= hi
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (d >= levels[mid]) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_ph_levels(uint32_t n, const double* __restrict__ rl, double max_rl, const double* __restrict__ levels,
                                                   uint32_t n_levels, unsigned long long* __restrict__ hist) {
    __shared__ uint32_t s_hist[PH_MAX_LEVELS + 1];
    if (n_levels > PH_MAX_LEVELS) return;   // (the host refused it)
    for (uint32_t t = threadIdx.x; t <= n_levels; t += blockDim.x) s_hist[t] = 0;
    __syncthreads();
    for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n; x += gridDim.x * blockDim.x)
        atomicAdd(&s_hist[ph_survived(rl[x] - max_rl, levels, n_levels)], 1u);
    __syncthreads();
    for (uint32_t t = threadIdx.x; t <= n_levels; t += blockDim.x)
        if (s_hist[t]) atomicAdd(&hist[t], (unsigned long long)s_hist[t]);
}

__global__ __launch_bounds__(256) void k_ph_survive(uint32_t n, const double* __restrict__ rl, double max_rl, double level,
                                                    uint8_t* __restrict__ keep) {
    for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n; x += gridDim.x * blockDim.x) keep[x] = (rl[x] - max_rl) >= level;
}

}  // namespace po
