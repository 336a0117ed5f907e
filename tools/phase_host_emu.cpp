// Host emulation of phasm_amd/csrc/phase.hip.h for tests/test_phase_host_emulation.py: the kernels compiled as plain C++ with
// ONE lane per wave and ONE thread per workgroup (threads run one after another, so a workgroup's LDS hand-offs need a
// workgroup of one), so a machine without a GPU checks their indexing and logic -- the bitsets, the intervals, the table
// tile by tile, the digits, the start-of-block test, the multinomial, the filter, the places, the level histogram and the
// survivors -- against the goldens, under the host sanitizers.
// The launches follow run_phase of c_api.hip: the same memsets, the same bounds, the same choice of the level.  The
// workspaces start as a call before could have left them.  Every loop here and in the kernels is bounded by a count.
//   stdin:  k P C R n_b start min_span prune max_candidates n_levels threshold, then overlap_max[R], aln_off[R+1], aln_b, aln_a0,
//           aln_a1, path_off[P+1], path_ids, set_off[C*k+1], set_ids, levels[n_levels]
//   stdout: "n_extensions n_kept n_out level_used"; the kept list "cand ext rl;"...; the list that comes out (the survivors
//           with prune, else the kept list again); the table.  Doubles as hexadecimal floats.
#include "host_emu.h"
#include <cmath>
#include <cstdlib>
#include <string>
#include "../phasm_amd/csrc/phase.hip.h"
using namespace po;

template <class T>
static bool read_n(std::vector<T>& v, size_t n, const char* fmt) {
    v.assign(n + 1, (T)0);
    for (size_t i = 0; i < n; ++i)
        if (scanf(fmt, &v[i]) != 1) return false;
    return true;
}

static void print_list(const std::vector<uint32_t>& c, const std::vector<uint32_t>& e, const std::vector<double>& r, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) printf("%u %u %a;", c[i], e[i], r[i]);
    printf("\n");
}

int main() {
    uint32_t k, P, C, R, nb, start, min_span, prune, max_cand, L;
    double threshold;
    if (scanf("%u %u %u %u %u %u %u %u %u %u %lf", &k, &P, &C, &R, &nb, &start, &min_span, &prune, &max_cand, &L, &threshold) != 11) return 1;
    if (k < 1 || k > PH_MAX_K || P < 1 || P > PH_MAX_P || !C || L > PH_MAX_LEVELS) return 1;
    uint64_t Pk64 = 1;
    for (uint32_t i = 0; i < k; ++i) Pk64 *= P;
    if (Pk64 * C >= (1ull << 31)) return 1;
    const uint32_t Pk = (uint32_t)Pk64, N = C * Pk, n_slots = C * k, W = std::max(1u, (nb + 31) / 32);
    std::vector<int32_t> om, a0, a1;
    std::vector<uint32_t> aln_off, aln_b, poff, pids, soff, sids;
    std::vector<double> levels;
    if (!read_n(om, R, "%d") || !read_n(aln_off, R + 1, "%u")) return 1;
    const uint32_t n_aln = aln_off[R];
    if (!read_n(aln_b, n_aln, "%u") || !read_n(a0, n_aln, "%d") || !read_n(a1, n_aln, "%d") || !read_n(poff, P + 1, "%u")) return 1;
    if (!read_n(pids, poff[P], "%u") || !read_n(soff, n_slots + 1, "%u") || !read_n(sids, soff[n_slots], "%u")) return 1;
    if (!read_n(levels, L, "%lf")) return 1;
    const size_t Rr = std::max<size_t>(R, 1);
    std::vector<uint32_t> sbits((size_t)n_slots * W, 0u), pbits((size_t)P * W, 0u), place(N + 1, 0xDEADu);
    std::vector<PhInterval> siv(n_slots * Rr, PhInterval{-7, -7}), piv(P * Rr, PhInterval{-7, -7});
    std::vector<double> table((size_t)n_slots * P, -7.0), rl(N + 1, -7.0);
    std::vector<uint8_t> keep(N + 1, 9);
    unsigned long long cnt[16] = {};
    LAUNCH(3, 1, k_ph_bits(n_slots, soff.data(), sids.data(), nb, W, sbits.data()));
    LAUNCH(3, 1, k_ph_bits(P, poff.data(), pids.data(), nb, W, pbits.data()));
    if (R) {
        LAUNCH(3, 1, k_ph_intervals(n_slots, R, nb, W, sbits.data(), aln_off.data(), aln_b.data(), a0.data(), a1.data(), om.data(), siv.data()));
        LAUNCH(3, 1, k_ph_intervals(P, R, nb, W, pbits.data(), aln_off.data(), aln_b.data(), a0.data(), a1.data(), om.data(), piv.data()));
    }
    LAUNCH(2, 1, k_ph_table(n_slots, P, R, siv.data(), piv.data(), om.data(), table.data()));
    PhExtend X;
    X.C = C; X.P = P; X.k = k; X.Pk = Pk;
    X.chunks = Pk;   // (a workgroup of one thread: a chunk is one extension)
    X.start_mode = start != 0;
    X.dead = R < min_span;
    X.kfact = 1;
    for (uint32_t i = 2; i <= k; ++i) X.kfact *= i;
    X.denom = (double)k * (double)R;
    X.log_thr = threshold == 0.0 ? -(double)INFINITY : std::log10(threshold);
    LAUNCH(5, 1, k_ph_extend(X, table.data(), rl.data(), keep.data(), cnt));
    uint32_t n_kept = 0;
    for (uint32_t x = 0; x < N; ++x) { place[x] = n_kept; n_kept += keep[x]; }   // (the library's prefix_sum over the bytes)
    if (n_kept != cnt[PK_KEPT] || n_kept > cnt[PK_ENUM] || cnt[PK_ENUM] > N) { printf("bound extensions\n"); return 0; }
    std::vector<uint32_t> kcand(n_kept + 1, 0xDEADu), kext(n_kept + 1, 0xDEADu), place2(n_kept + 1, 0xDEADu);
    std::vector<double> krl(n_kept + 1, -7.0);
    std::vector<uint8_t> keep2(n_kept + 1, 9);
    double max_rl = std::nan("");
    if (n_kept) {
        LAUNCH(3, 1, k_ph_gather(N, n_kept, Pk, keep.data(), place.data(), (const uint32_t*)nullptr, (const uint32_t*)nullptr, rl.data(),
                                 kcand.data(), kext.data(), krl.data(), cnt + PK_N));
        const unsigned long long key = cnt[PK_N];
        if (!key) { printf("bound greatest\n"); return 0; }
        const unsigned long long bits = (key >> 63) ? (key & 0x7FFFFFFFFFFFFFFFull) : ~key;
        memcpy(&max_rl, &bits, 8);
    }
    std::vector<uint32_t> scand(n_kept + 1, 0xDEADu), sext(n_kept + 1, 0xDEADu);
    std::vector<double> srl(n_kept + 1, -7.0);
    const std::vector<uint32_t>*fc = &kcand, *fe = &kext;
    const std::vector<double>* fr = &krl;
    uint32_t n_final = n_kept;
    int level_used = -1;
    if (prune && n_kept >= 2 && L && max_rl != -(double)INFINITY) {
        std::vector<double> lv(levels.begin(), levels.begin() + L);
        for (uint32_t j = 1; j < L; ++j) lv[j] = lv[j] >= lv[j - 1] ? lv[j] : lv[j - 1];
        std::vector<unsigned long long> hist(L + 1, 0xDEADull);
        std::fill(hist.begin(), hist.end(), 0ull);   // (the memset of run_phase)
        LAUNCH(3, 1, k_ph_levels(n_kept, krl.data(), max_rl, lv.data(), L, hist.data()));
        std::vector<unsigned long long> left(L);
        unsigned long long behind = 0, all = hist[0];
        for (uint32_t j = L; j-- > 0;) { behind += hist[j + 1]; left[j] = behind; all += hist[j + 1]; }
        if (all != n_kept) { printf("bound levels\n"); return 0; }
        uint32_t used = L - 1;
        for (uint32_t j = 0; j < L; ++j) if (left[j] <= max_cand) { used = j; break; }
        level_used = (int)used;
        LAUNCH(3, 1, k_ph_survive(n_kept, krl.data(), max_rl, lv[used], keep2.data()));
        uint32_t n_left = 0;
        for (uint32_t x = 0; x < n_kept; ++x) { place2[x] = n_left; n_left += keep2[x]; }
        if (n_left != left[used]) { printf("bound survivors\n"); return 0; }
        if (n_left) LAUNCH(3, 1, k_ph_gather(n_kept, n_left, Pk, keep2.data(), place2.data(), kcand.data(), kext.data(), krl.data(), scand.data(),
                                             sext.data(), srl.data(), (unsigned long long*)nullptr));
        fc = &scand; fe = &sext; fr = &srl;
        n_final = n_left;
    }
    printf("%llu %u %u %d\n", cnt[PK_ENUM], n_kept, n_final, level_used);
    print_list(kcand, kext, krl, n_kept);
    print_list(*fc, *fe, *fr, n_final);
    for (size_t i = 0; i < table.size(); ++i) printf("%a ", table[i]);
    printf("\n");
    return 0;
}
