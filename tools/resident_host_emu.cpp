// Host emulation of phasm_amd/csrc/resident.hip.h for tests/test_resident_host_emulation.py: the k_rs_ kernels compiled as plain
// C++ with ONE lane per wave (threads run one after another), so a machine without a GPU checks their indexing and logic -- the
// numbering of the reads new to a block, the translation of aln_b and of the path ids, the commit of the map and of the two
// previous sets, the lazy clear after a reset -- under the host sanitizers.  The launches follow rs_prepare,
// run_walk_step_resident and run_walk_prev_copy of c_api.hip; what the gather (relevant.hip.h, with an emulator of its own)
// leaves for them -- b_reads, aln_b, the words of cur_graph, cur_aligning and G and the ranks of G -- is made here from the
// lists of the event.  Every scratch array has exactly the length the library gives it and starts as garbage.  Every loop here
// and in the kernels is bounded by a count.
//   stdin:  n_ids, then events until the end of the input:
//             "S advance  n_cur cur..  n_ca ca..  n_b b..  n_aln aln_b..  P  then per path: len id.."
//                 one gather and its step: cur_graph (duplicates allowed), cur_aligning, b_reads (strictly ascending), aln_b
//                 (local ids), the path reads (global ids); advance 1: the step took its list over
//             "R"  po_walk_reset
//   stdout: after an S event eight lines: "n_new nb"; the translation local -> stable; aln_b rewritten; the path ids
//           rewritten; "n_block" and global_of; the pairs global:stable of stable_of; prev_graph; prev_aligning.
//           After an R event the line "reset" (nothing on the device is touched).
//   An event the library would refuse (an id at or above n_ids, b_reads not strictly ascending, a local id at or above n_b,
//   P outside 1..64, a b read that is not in cur_graph or prev_graph) ends the program with status 1.
#include "host_emu.h"
#include <cstdlib>
#define __popc __builtin_popcount
#include "../phasm_amd/csrc/resident.hip.h"
using namespace po;

static bool read_list(std::vector<uint32_t>& out, uint32_t below) {
    uint32_t n;
    if (scanf("%u", &n) != 1 || n > (1u << 24)) return false;
    out.resize(n);
    for (uint32_t j = 0; j < n; ++j)
        if (scanf("%u", &out[j]) != 1 || out[j] >= below) return false;
    return true;
}

static void print_list(const std::vector<uint32_t>& v, size_t n) {
    for (size_t j = 0; j < n; ++j) printf("%u ", v[j]);
    printf("\n");
}

int main() {
    uint32_t n_ids;
    if (scanf("%u", &n_ids) != 1 || n_ids < 1 || n_ids > (1u << 24)) return 1;
    const uint32_t W = (n_ids + 31) / 32;
    const size_t Wp = (size_t)W + 1;
    // the walk's device state: made at the first device call (rs_prepare), garbage before
    std::vector<uint32_t> prev(2 * Wp, 0xDEADBEEFu), stable_of((size_t)n_ids + 1, 0xDEADBEEFu), global_of;
    bool ready = false, clear_prev = false;
    uint32_t n_block = 0, unmap_n = 0;
    char what;
    while (scanf(" %c", &what) == 1) {
        if (what == 'R') {   // (walk_clear: the host notes what the next device call has to clear)
            if (n_block) {
                unmap_n = n_block;
                n_block = 0;
            }
            clear_prev = ready;
            printf("reset\n");
            continue;
        }
        if (what != 'S') return 1;
        uint32_t advance, P;
        std::vector<uint32_t> cur, ca_list, b_reads, aln_b;
        if (scanf("%u", &advance) != 1 || advance > 1) return 1;
        if (!read_list(cur, n_ids) || !read_list(ca_list, n_ids) || !read_list(b_reads, n_ids)) return 1;
        const uint32_t n_b = (uint32_t)b_reads.size();
        for (uint32_t j = 1; j < n_b; ++j)
            if (b_reads[j] <= b_reads[j - 1]) return 1;
        if (!read_list(aln_b, n_b ? n_b : 1) || (!n_b && !aln_b.empty())) return 1;
        if (scanf("%u", &P) != 1 || P < 1 || P > 64) return 1;
        std::vector<uint32_t> poff(P + 1, 0), pin;
        for (uint32_t p = 0; p < P; ++p) {
            std::vector<uint32_t> one;
            if (!read_list(one, n_ids)) return 1;
            pin.insert(pin.end(), one.begin(), one.end());
            poff[p + 1] = (uint32_t)pin.size();
        }
        const uint32_t n_aln = (uint32_t)aln_b.size(), n_pids = (uint32_t)pin.size();
        // rs_prepare
        if (!ready) {
            std::fill(prev.begin(), prev.end(), 0u);
            std::fill(stable_of.begin(), stable_of.end(), RS_NONE);
            ready = true;
            unmap_n = 0;
            clear_prev = false;
        } else {
            if (unmap_n) {
                LAUNCH(3, 2, k_rs_unmap(unmap_n, global_of.data(), n_ids, stable_of.data()));
                unmap_n = 0;
            }
            if (clear_prev) {
                std::fill(prev.begin(), prev.end(), 0u);
                clear_prev = false;
            }
        }
        // what the gather leaves in the walk's buffers: the words of cur_aligning, cur_graph and G, the ranks of G
        std::vector<uint32_t> bits(6 * Wp, 0u), g_rank(Wp, 0xDEADBEEFu);
        uint32_t *ca = bits.data(), *gc = bits.data() + 2 * Wp, *g = bits.data() + 5 * Wp;
        for (uint32_t x : ca_list) ca[x >> 5] |= 1u << (x & 31);
        for (uint32_t x : cur) gc[x >> 5] |= 1u << (x & 31);
        for (uint32_t x : b_reads) {
            if (!((gc[x >> 5] | prev[x >> 5]) >> (x & 31) & 1u)) return 1;   // (G is cur_graph + prev_graph, or less)
            g[x >> 5] |= 1u << (x & 31);
        }
        uint32_t run = 0;
        for (uint32_t w = 0; w < W; ++w) {
            g_rank[w] = run;
            run += (uint32_t)__builtin_popcount(g[w]);
        }
        g_rank[W] = run;
        // run_walk_step_resident up to the scoring
        std::vector<uint32_t> flag((size_t)n_b + 1, 0xDEADBEEFu), rank((size_t)n_b + 2, 0xDEADBEEFu), xl((size_t)n_b + 1, 0xDEADBEEFu),
            alnb((size_t)n_aln + 1, 0xDEADBEEFu), pids((size_t)n_pids + 1, 0xDEADBEEFu);
        pin.push_back(0xDEADBEEFu);
        uint32_t n_new = 0;
        if (n_b) {
            LAUNCH(3, 2, k_rs_flag(n_b, b_reads.data(), n_ids, stable_of.data(), flag.data()));
            for (uint32_t j = 0; j < n_b; ++j) {   // (the library's prefix_sum: exclusive, the total behind the last)
                if (flag[j] > 1) return 2;
                rank[j] = n_new;
                n_new += flag[j];
            }
            rank[n_b] = n_new;
        }
        const uint32_t nb = n_block + n_new;
        if (n_b) {
            LAUNCH(3, 2, k_rs_local(n_b, b_reads.data(), n_ids, stable_of.data(), n_block, flag.data(), rank.data(), xl.data()));
            if (n_aln) LAUNCH(3, 2, k_rs_alnb(n_aln, aln_b.data(), n_b, xl.data(), alnb.data()));
        }
        if (n_pids) {
            if (n_b)
                LAUNCH(3, 2, k_rs_paths(n_pids, pin.data(), n_ids, g, g_rank.data(), n_b, xl.data(), pids.data()));
            else
                std::fill(pids.begin(), pids.begin() + n_pids, RS_NONE);
        }
        if (advance) {
            global_of.resize((size_t)nb + 1, 0xDEADBEEFu);   // (walk_grow keeps the first n_block entries)
            if (n_new) LAUNCH(3, 2, k_rs_commit(n_b, b_reads.data(), n_ids, flag.data(), xl.data(), nb, stable_of.data(), global_of.data()));
            LAUNCH(3, 2, k_rs_or(W, gc, ca, prev.data(), prev.data() + Wp));
            n_block = nb;
        }
        // the outputs of the event and the state behind it
        printf("%u %u\n", n_new, nb);
        print_list(xl, n_b);
        print_list(alnb, n_aln);
        print_list(pids, n_pids);
        printf("%u ", n_block);
        print_list(global_of, n_block);
        for (uint32_t x = 0; x < n_ids; ++x)
            if (stable_of[x] != RS_NONE) printf("%u:%u ", x, stable_of[x]);
        printf("\n");
        for (int which = 0; which < 2; ++which) {   // (run_walk_prev_copy: the counts, the library's prefix_sum, k_rr_list)
            std::vector<uint32_t> cnt(Wp, 0xDEADBEEFu);
            const uint32_t* set = prev.data() + (which ? Wp : 0);
            LAUNCH(2, 3, k_rs_popc(W, set, cnt.data()));
            for (uint32_t w = 0; w < W; ++w) {
                if (cnt[w] > 32) return 2;
                for (uint32_t b = 0; b < 32; ++b)
                    if ((set[w] >> b) & 1u) printf("%u ", w * 32 + b);
            }
            uint32_t total = 0, bits_set = 0;
            for (uint32_t w = 0; w < W; ++w) {
                total += cnt[w];
                bits_set += (uint32_t)__builtin_popcount(set[w]);
            }
            if (total != bits_set) return 2;
            printf("\n");
        }
    }
    return 0;
}
