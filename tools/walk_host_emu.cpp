// Host emulation of phasm_amd/csrc/walk.hip.h for tests/test_walk_host_emulation.py: the kernels compiled as plain C++ with
// ONE lane per wave (threads run one after another), so a machine without a GPU checks their indexing and logic -- the rows
// of the ping-pong pair as they grow and shrink, the digits of an extension id, the links and their trace-back, the greatest
// log_rl and the tie set -- under the host sanitizers.  The launches follow run_walk_step, run_walk_best and
// run_walk_history of c_api.hip: the other half of the pair is sized for the new list and starts as garbage, the links grow
// behind those of the depths before.  Every loop here and in the kernels is bounded by a count.
//   stdin:  k, then events until the end of the input:
//             "A P nb n_new", then per path "len id.." (block-stable ids below nb), then n_new times "cand ext rl" (rl as a
//             hexadecimal float): the survivors of a step become the state
//             "R": po_walk_reset
//           every event is followed by a snapshot on stdout:
//             "n_cands W depth"; the rows, one slot per ";"-ended group of W hexadecimal words; the extension ids of every
//             candidate, oldest first, one candidate per ";"; the tie set
#include "host_emu.h"
#include <cmath>
#include <cstdlib>
#include "../phasm_amd/csrc/phase.hip.h"
#include "../phasm_amd/csrc/walk.hip.h"
using namespace po;

int main() {
    uint32_t k;
    if (scanf("%u", &k) != 1 || k < 1 || k > PH_MAX_K) return 1;
    std::vector<uint32_t> rows[2];
    std::vector<double> rl[2];
    std::vector<WkLink> links;
    std::vector<unsigned long long> level_off;
    uint32_t n_cands = 1, W = 0, n_block = 0;
    int cur = 0;
    char what;
    while (scanf(" %c", &what) == 1) {
        if (what == 'R') {
            n_cands = 1; W = 0; n_block = 0;
            level_off.clear();
        } else if (what == 'A') {
            uint32_t P, nb, n_new;
            if (scanf("%u %u %u", &P, &nb, &n_new) != 3 || P < 1 || P > PH_MAX_P || nb < n_block || !n_new) return 1;
            std::vector<uint32_t> poff(P + 1, 0), pids;
            for (uint32_t p = 0; p < P; ++p) {
                uint32_t len;
                if (scanf("%u", &len) != 1) return 1;
                for (uint32_t j = 0; j < len; ++j) {
                    uint32_t id;
                    if (scanf("%u", &id) != 1 || id >= nb) return 1;
                    pids.push_back(id);
                }
                poff[p + 1] = (uint32_t)pids.size();
            }
            pids.push_back(0);
            std::vector<uint32_t> cand(n_new), ext(n_new);
            std::vector<double> srl(n_new);
            uint64_t Pk = 1;
            for (uint32_t i = 0; i < k; ++i) Pk *= P;
            for (uint32_t j = 0; j < n_new; ++j)
                if (scanf("%u %u %lf", &cand[j], &ext[j], &srl[j]) != 3 || cand[j] >= n_cands || ext[j] >= Pk) return 1;
            const uint32_t W_new = std::max(1u, (nb + 31) / 32), depth = level_off.empty() ? 0u : (uint32_t)level_off.size() - 1;
            std::vector<uint32_t> pbits((size_t)P * W_new, 0u);   // (the memset of run_phase)
            LAUNCH(3, 1, k_ph_bits(P, poff.data(), pids.data(), nb, W_new, pbits.data()));
            const int nxt = cur ^ 1;
            const unsigned long long used = depth ? level_off[depth] : 0;
            rows[nxt].assign((size_t)n_new * k * W_new, 0xDEADBEEFu);   // (whatever two steps ago left there)
            rl[nxt].assign(n_new, -7.0);
            links.resize(used + n_new, WkLink{0xDEADu, 0xDEADu});
            LAUNCH(3, 2, k_wk_advance(n_new, n_cands, k, P, W, W_new, rows[cur].data(), pbits.data(), cand.data(), ext.data(), srl.data(),
                                      rows[nxt].data(), links.data() + used, rl[nxt].data()));
            if (level_off.empty()) level_off.push_back(0);
            level_off.push_back(used + n_new);
            cur = nxt;
            n_cands = n_new;
            W = W_new;
            n_block = nb;
        } else {
            return 1;
        }
        // the snapshot
        const uint32_t depth = level_off.empty() ? 0u : (uint32_t)level_off.size() - 1;
        printf("%u %u %u\n", n_cands, depth ? W : 0u, depth);
        if (depth)
            for (size_t s = 0; s < (size_t)n_cands * k; ++s) {
                for (uint32_t w = 0; w < W; ++w) printf("%x ", rows[cur][s * W + w]);
                printf(";");
            }
        printf("\n");
        if (depth) {
            std::vector<uint32_t> all(n_cands), out((size_t)n_cands * depth, 0xDEADu);
            for (uint32_t c = 0; c < n_cands; ++c) all[c] = c;
            LAUNCH(2, 2, k_wk_trace(n_cands, depth, level_off.data(), links.data(), all.data(), out.data()));
            for (uint32_t c = 0; c < n_cands; ++c) {
                for (uint32_t d = 0; d < depth; ++d) printf("%u ", out[(size_t)c * depth + d]);
                printf(";");
            }
        }
        printf("\n");
        bool everyone = depth == 0 || n_cands < 2;
        double max_rl = -(double)INFINITY;
        if (depth) {
            unsigned long long key = 0;
            LAUNCH(3, 1, k_wk_max(n_cands, rl[cur].data(), &key));
            if (!key) { printf("bound greatest\n"); return 0; }
            const unsigned long long bits = (key >> 63) ? (key & 0x7FFFFFFFFFFFFFFFull) : ~key;
            memcpy(&max_rl, &bits, 8);
            everyone = everyone || max_rl == -(double)INFINITY;
        }
        if (everyone) {
            for (uint32_t c = 0; c < n_cands; ++c) printf("%u ", c);
        } else {
            std::vector<uint8_t> keep(n_cands + 1, 9);
            std::vector<uint32_t> place(n_cands + 1, 0xDEADu), out(n_cands + 1, 0xDEADu);
            LAUNCH(3, 1, k_ph_survive(n_cands, rl[cur].data(), max_rl, 0.0, keep.data()));
            uint32_t n_best = 0;
            for (uint32_t x = 0; x < n_cands; ++x) { place[x] = n_best; n_best += keep[x]; }   // (the library's prefix_sum over the bytes)
            LAUNCH(3, 1, k_wk_pick(n_cands, n_best, keep.data(), place.data(), out.data()));
            for (uint32_t j = 0; j < n_best; ++j) printf("%u ", out[j]);
        }
        printf("\n");
    }
    return 0;
}
