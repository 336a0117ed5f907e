// Host emulation of phasm_amd/csrc/large.hip.h for tests/test_large_host_emulation.py: the kernels compiled as plain C++ with
// ONE lane per wave and ONE thread per workgroup (threads run one after another, so a workgroup's LDS hand-offs need a
// workgroup of one), so a machine without a GPU checks their indexing and logic -- the slot map, the bitsets and intervals of
// the interior nodes (k_ph_bits and k_ph_intervals of phase.hip.h, as the call launches them), the join along a path chunk by
// chunk and tile by tile, the division, the rounds of the selection -- against the goldens, under the host sanitizers.
// The launches follow run_large of c_api.hip: the same memsets, the same bounds, the same checks in front (a refused call ends
// the program with status 1).  The workspaces start as a call before could have left them.  Every loop is bounded by a count.
//   stdin:  n_total n_inside P R n_b n_best, then inside_nodes[n_inside], path_off[P+1] (relative to the bubble's first path),
//           path_nodes, overlap_max[R], aln_off[R+1], aln_b, aln_a0, aln_a1, node_off[n_inside+1], node_ids
//   stdout: "n_best max_path_nodes"; the best list "index score;"...; every score.  Doubles as hexadecimal floats.
#include "host_emu.h"
#include <cmath>
#include <cstdlib>
#include <string>
#include "../phasm_amd/csrc/phase.hip.h"
#include "../phasm_amd/csrc/large.hip.h"
using namespace po;

template <class T>
static bool read_n(std::vector<T>& v, size_t n, const char* fmt) {
    v.assign(n + 1, (T)0);
    for (size_t i = 0; i < n; ++i)
        if (scanf(fmt, &v[i]) != 1) return false;
    return true;
}

static bool ascending(const std::vector<uint32_t>& off, size_t n) {
    if (off[0] != 0) return false;
    for (size_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return false;
    return true;
}

int main() {
    uint32_t n_total, n_inside, P, R, nb, n_best;
    if (scanf("%u %u %u %u %u %u", &n_total, &n_inside, &P, &R, &nb, &n_best) != 6) return 1;
    if (n_best < 1 || n_best > LG_MAX_BEST || !R || !P) return 1;
    std::vector<uint32_t> inside, poff, pnodes, aln_off, aln_b, noff, nids;
    std::vector<int32_t> om, a0, a1;
    if (!read_n(inside, n_inside, "%u") || !read_n(poff, P + 1, "%u") || !ascending(poff, P) || !read_n(pnodes, poff[P], "%u")) return 1;
    if (!read_n(om, R, "%d") || !read_n(aln_off, R + 1, "%u") || !ascending(aln_off, R)) return 1;
    const uint32_t n_aln = aln_off[R];
    if (!read_n(aln_b, n_aln, "%u") || !read_n(a0, n_aln, "%d") || !read_n(a1, n_aln, "%d")) return 1;
    if (!read_n(noff, n_inside + 1, "%u") || !ascending(noff, n_inside) || !read_n(nids, noff[n_inside], "%u")) return 1;
    for (uint32_t j = 0; j < n_aln; ++j)
        if (aln_b[j] >= nb) return 1;
    for (uint32_t j = 0; j < noff[n_inside]; ++j)
        if (nids[j] >= nb) return 1;
    const uint32_t W = std::max(1u, (nb + 31) / 32);
    // (sized exactly: a step past an end is the sanitizer's to find)
    inside.resize(n_inside);
    pnodes.resize(poff[P]);
    std::vector<uint32_t> nbits((size_t)n_inside * W, 0xDEADu), slot_of(n_total, 0xDEADu);
    std::vector<PhInterval> niv((size_t)n_inside * R, PhInterval{-7, -7});
    std::vector<double> score(P, -7.0);
    unsigned long long cnt[LK_N];
    for (unsigned long long& c : cnt) c = 0xDEADull;
    std::fill(cnt, cnt + LK_BEST, 0ull);                     // (the memsets of run_large)
    std::fill(cnt + LK_BEST, cnt + LK_N, LG_NO_INDEX);
    std::fill(slot_of.begin(), slot_of.end(), LG_NO_SLOT);
    std::fill(nbits.begin(), nbits.end(), 0u);
    if (n_inside) {
        LAUNCH(3, 1, k_lg_slots(n_inside, inside.data(), n_total, slot_of.data()));
        LAUNCH(3, 1, k_ph_bits(n_inside, noff.data(), nids.data(), nb, W, nbits.data()));
        LAUNCH(3, 1, k_ph_intervals(n_inside, R, nb, W, nbits.data(), aln_off.data(), aln_b.data(), a0.data(), a1.data(), om.data(), niv.data()));
    }
    LAUNCH(3, 1, k_lg_score(P, R, n_inside, n_total, poff.data(), pnodes.data(), slot_of.data(), niv.data(), om.data(), score.data(), cnt));
    const uint32_t n = n_best < P ? n_best : P;
    for (uint32_t j = 0; j < n; ++j) {
        LAUNCH(3, 1, k_lg_best_key(P, j, score.data(), cnt));
        LAUNCH(3, 1, k_lg_best_idx(P, j, score.data(), cnt));
    }
    printf("%u %llu\n", n, cnt[LK_MAXLEN]);
    for (uint32_t j = 0; j < n; ++j) {
        const unsigned long long key = cnt[LK_KEY + j], at = cnt[LK_BEST + j];
        if (!key || at >= P) { printf("bound selection\n"); return 0; }
        const unsigned long long bits = (key >> 63) ? (key & 0x7FFFFFFFFFFFFFFFull) : ~key;
        double s;
        memcpy(&s, &bits, 8);
        printf("%llu %a;", at, s);
    }
    printf("\n");
    for (uint32_t p = 0; p < P; ++p) printf("%a ", score[p]);
    printf("\n");
    return 0;
}
