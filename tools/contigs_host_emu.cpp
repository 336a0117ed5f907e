// Host emulation of phasm_amd/csrc/contigs.hip.h for tests/test_contigs_host_emulation.py: the kernels compiled as plain C++
// with ONE lane per wave (threads run one after another), so a machine without a GPU checks their indexing and logic --
// behind the ranks (the kernels of components.hip.h, as ranked_open of c_api.hip launches them: rank_host_emu.h), with the
// exclude bytes given (the other way to them, the bubble-chain stage, is bubblechains_host_emu.cpp's): degrees and the one
// in-edge, the class of every edge, the ranking rounds between two buffer triples, the coverage rounds between two buffer
// pairs, the sums at the heads, the filter, the sort of the surviving heads, the table and the two arrays -- against the
// goldens, under the host sanitizers.
// The launches follow run_contigs: the same memsets, the same bounds, the batches and the stop at the first round that
// resolves nothing from round_phase of components.hip.h.  The workspaces start as a call before could have left them.  Every
// loop here and in the kernels is bounded by a count.
//   argv:   min_contig_len (default 5000), n_ids (default n_total: ids at or above it are merged nodes)
//   stdin:  n_total n_edges n_order, one "u v weight" line per edge, the nodes in node order, their lengths in node order,
//           their exclude bytes in node order
//   stdout: "invalid N" alone, "bound WHAT" alone, or: order, excluded, root starts, late starts, blocked, covered, uncovered,
//           paths, short paths, isolated, short isolated, contigs, nodes of the longest path; ranking rounds, coverage rounds,
//           batches, the largest batch; the contig of every edge (as given); the place of every edge; per contig
//           "first_node last_node n_nodes first_edge length;"
#include "host_emu.h"
#include <cstdlib>
namespace po {
struct Edge { uint32_t u, v; int32_t weight, overlap_len; };
constexpr unsigned long long NODE_NO_RANK = ~0ull;
}
#include "../phasm_amd/csrc/merge.hip.h"
#include "../phasm_amd/csrc/components.hip.h"
#include "../phasm_amd/csrc/contigs.hip.h"
using namespace po;

#include "rank_host_emu.h"

// what round_phase clears and reads back, for a host that runs every launch at once
struct Batches {
    unsigned long long rcnt[CC_BATCH] = {};
    uint32_t batches = 0, max_batch = 0, noted = 0;
    void note(uint32_t j) { noted = j + 1 > noted ? j + 1 : noted; }
    bool begin(uint32_t batch) { for (uint32_t j = 0; j < batch && j < CC_BATCH; ++j) rcnt[j] = 0; noted = 0; return batch <= CC_BATCH; }
    bool end(uint32_t batch, const volatile uint64_t*& words) {
        static uint64_t home[CC_BATCH];
        for (uint32_t j = 0; j < batch; ++j) home[j] = rcnt[j];
        words = home;
        max_batch = noted > max_batch ? noted : max_batch;
        return noted == batch;
    }
};

int main(int argc, char** argv) {
    const unsigned long long min_len = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 5000ull;
    RankedInput g;
    std::vector<uint32_t> ine;
    const int status = ranked_input(g, ine, true);   // (the identity words: overwritten below, as in run_contigs)
    if (status >= 0) return status;
    const uint32_t n = g.n, n_order = g.n_order, nn = g.nn, n_total = g.n_total;
    const uint32_t n_ids = argc > 2 ? (uint32_t)std::strtoul(argv[2], nullptr, 10) : n_total;
    if (n_ids > n_total) return 1;
    const std::vector<EdgeRanks>& ends = g.ends;
    std::vector<uint32_t> len(n_ids + 1, 0xDEADu);
    std::vector<long long> mlen(n_total - n_ids + 1, 0xDEADll);
    std::vector<uint8_t> excl(nn, 9);
    for (uint32_t r = 0; r < n_order; ++r) {
        long long x;
        if (scanf("%lld", &x) != 1) return 1;
        const uint32_t id = g.val[r];
        if (id < n_ids) len[id] = (uint32_t)x; else mlen[id - n_ids] = x;
    }
    for (uint32_t r = 0; r < n_order; ++r) { uint32_t x; if (scanf("%u", &x) != 1) return 1; excl[r] = (uint8_t)x; }
    if (!n_order) { printf("0 0 0 0 0 0 0 0 0 0 0 0 0\n0 0 0 0\n\n\n\n"); return 0; }
    // ---- the contigs, as run_contigs launches them
    const size_t ne = (size_t)n + 1;
    const uint32_t pad_e = merge_sort_pad((uint32_t)ne);
    std::vector<uint32_t> indeg(nn, 0xDEADu), outdeg(nn, 0xDEADu), jb0(ne, 0xDEADu), jb1(ne, 0xDEADu), hops0(ne, 0xDEADu), hops1(ne, 0xDEADu),
        cj0(ne, 0xDEADu), cj1(ne, 0xDEADu), head_of(ne, 0xDEADu), pn(ne, 0xDEADu), plast(ne, 0xDEADu), val(pad_e, 0xDEADu), d_contig(ne, 0xDEADu),
        d_pos(ne, 0xDEADu);
    std::vector<unsigned long long> ws0(ne, 0xDEADull), ws1(ne, 0xDEADull), key(pad_e, 7);
    std::vector<long long> nlen(nn, 0xDEADll), plen(ne, 0xDEADll);
    std::vector<uint8_t> cls(ne, 9), ok0(ne, 9), ok1(ne, 9), kept(ne, 9);
    std::vector<Contig> table(nn + ne, Contig{0xDEADu, 0xDEADu, 0xDEADu, 0xDEADu, 0xDEADll});
    uint32_t *jb[2] = {jb0.data(), jb1.data()}, *hops[2] = {hops0.data(), hops1.data()}, *cj[2] = {cj0.data(), cj1.data()};
    unsigned long long* ws[2] = {ws0.data(), ws1.data()};
    uint8_t* ok[2] = {ok0.data(), ok1.data()};
    unsigned long long tc[16] = {};
    LAUNCH(3, 4, k_ct_init(n_order, g.val.data(), n_ids, n_total, len.data(), n_ids < n_total ? mlen.data() : nullptr, nullptr, excl.data(),
                           indeg.data(), outdeg.data(), ine.data(), nlen.data(), tc));
    if (n) {
        LAUNCH(3, 4, k_ct_degrees(ends.data(), n, n_order, indeg.data(), outdeg.data(), ine.data()));
        LAUNCH(3, 4, k_ct_classes(ends.data(), n, n_order, indeg.data(), outdeg.data(), excl.data(), cls.data(), tc));
        LAUNCH(3, 4, k_ct_links(ends.data(), g.e.data(), n, n_order, ine.data(), cls.data(), jb[0], hops[0], ws[0]));
        std::fill(pn.begin(), pn.begin() + n, 0u);
    }
    Batches bops;
    uint64_t ignored = 0;
    uint32_t path_rounds = 0, cover_rounds = 0, launched = 0;
    if (n) {
        const int how = round_phase(bops, n, [&](uint32_t j) {
            bops.note(j);
            const uint32_t a = launched & 1, b = a ^ 1;
            LAUNCH(3, 4, k_ct_jump(n, jb[a], hops[a], ws[a], jb[b], hops[b], ws[b], bops.rcnt + j));
            ++launched;
        }, path_rounds, bops.batches, ignored);
        if (how != ROUNDS_DONE) { printf("bound ranking\n"); return 0; }
    }
    const uint32_t fin = launched & 1;
    launched = 0;
    if (n) {
        LAUNCH(3, 4, k_ct_cover_init(ends.data(), n, n_order, ine.data(), cls.data(), jb[fin], cj[0], ok[0]));
        const int how = round_phase(bops, n, [&](uint32_t j) {
            bops.note(j);
            const uint32_t a = launched & 1, b = a ^ 1;
            LAUNCH(3, 4, k_ct_cover_jump(n, cj[a], ok[a], cj[b], ok[b], bops.rcnt + j));
            ++launched;
        }, cover_rounds, bops.batches, ignored);
        if (how != ROUNDS_DONE) { printf("bound coverage\n"); return 0; }
    }
    const uint32_t cfin = launched & 1;
    uint32_t *eidx = jb[fin ^ 1], *cidx = cj[cfin ^ 1];
    if (n) {
        LAUNCH(3, 4, k_ct_paths(ends.data(), g.e.data(), n, n_order, indeg.data(), outdeg.data(), nlen.data(), cls.data(), jb[fin], hops[fin],
                                ws[fin], cj[cfin], ok[cfin], head_of.data(), pn.data(), plast.data(), plen.data(), tc));
        LAUNCH(3, 4, k_ct_filter(n, min_len, head_of.data(), pn.data(), plen.data(), kept.data(), tc));
    }
    LAUNCH(3, 4, k_ct_isolated(n_order, min_len, indeg.data(), outdeg.data(), nlen.data(), g.root.data(), tc));
    uint32_t n_kept = 0;
    for (uint32_t e = 0; e < n; ++e) { eidx[e] = n_kept; n_kept += kept[e]; }   // (the library's prefix_sum over the bytes)
    const uint32_t n_iso = number_roots(g);
    if (tc[TK_BAD]) { printf("bound last edge\n"); return 0; }
    if (tc[TK_COVERED] + tc[TK_UNCOVERED] != n || tc[TK_PEDGES] != tc[TK_COVERED] || n_kept != tc[TK_KEPT] || n_kept + tc[TK_SHORT] != tc[TK_PATHS] ||
        n_iso + tc[TK_SHORTISO] != tc[TK_ISO] || tc[TK_PATHS] > tc[TK_ROOT] + tc[TK_LATE] || tc[TK_ROOT] + tc[TK_LATE] > n || tc[TK_ISO] > n_order ||
        tc[TK_MAXN] > (uint64_t)n + 1) {
        printf("bound paths\n");
        return 0;
    }
    if (n_kept) {
        const uint32_t pad = merge_sort_pad(n_kept);
        if (pad > pad_e) { printf("bound pad\n"); return 0; }
        LAUNCH(3, 4, k_ct_keys(ends.data(), n, n_kept, pad, kept.data(), eidx, key.data(), val.data()));
        merge_sort_steps(n_kept, [&](uint32_t j, uint32_t k) { LAUNCH((pad + 3) / 4, 4, k_merge_bitonic(key.data(), val.data(), pad, j, k)); });
        LAUNCH(3, 4, k_ct_number(ends.data(), n, n_order, n_kept, val.data(), g.val.data(), pn.data(), plast.data(), plen.data(), cidx,
                                 table.data()));
    }
    if (n_iso) LAUNCH(3, 4, k_ct_iso_table(n_order, n_kept, n_iso, g.root.data(), g.index.data(), g.val.data(), nlen.data(), table.data()));
    if (n) LAUNCH(3, 4, k_ct_edge_out(n, head_of.data(), kept.data(), cidx, hops[fin], d_contig.data(), d_pos.data()));
    const uint32_t n_contigs = n_kept + n_iso;
    printf("%u %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %u %llu\n", n_order, tc[TK_EXCLUDED], tc[TK_ROOT], tc[TK_LATE], tc[TK_BLOCKED],
           tc[TK_COVERED], tc[TK_UNCOVERED], tc[TK_PATHS], tc[TK_SHORT], tc[TK_ISO], tc[TK_SHORTISO], n_contigs, tc[TK_MAXN]);
    printf("%u %u %u %u\n", path_rounds, cover_rounds, bops.batches, bops.max_batch);
    for (uint32_t e = 0; e < n; ++e) printf("%u ", d_contig[e]);
    printf("\n");
    for (uint32_t e = 0; e < n; ++e) printf("%u ", d_pos[e]);
    printf("\n");
    for (uint32_t i = 0; i < n_contigs; ++i)
        printf("%u %u %u %u %lld;", table[i].first_node, table[i].last_node, table[i].n_nodes, table[i].first_edge, table[i].length);
    printf("\n");
    return 0;
}
