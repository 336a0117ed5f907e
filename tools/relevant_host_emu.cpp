// Host emulation of phasm_amd/csrc/relevant.hip.h for tests/test_relevant_host_emulation.py: the kernels compiled as plain C++
// with ONE lane per wave and ONE thread per workgroup, so a machine without a GPU checks their indexing and logic -- the
// claim of a key and the winner by sequence number, the fill, the sort by rank, the places, the bitsets, the rank queries, the
// counted and written alignments, the look-ups of overlap_max -- against the goldens, under the host sanitizers.
// The launches follow run_phase_index and run_relevant of c_api.hip: the same memsets, the same bounds, the same decisions
// between the launches.  The workspaces start as a call before could have left them.  Every loop here and in the kernels is
// bounded by a count.
//   stdin:  n_ids n_rows n_slots n_queries (n_slots 0: the library's table size; else a table of that many slots -- a small one
//           makes the probe sequences wrap past its end), len[n_ids], the rows (6 numbers each), then per query
//           mode min_span n_cur n_prev_graph n_prev_aligning n_pred and the five lists
//   stdout: "n_keys max_degree n_invalid", the offsets, the entries (b a0 a1 seq each); per query "n_cur_aligning n_spanning
//           fell_back n_relevant n_alignments n_b" and eight lines: cur_aligning, rel_reads, overlap_max, aln_off, aln_b, aln_a0,
//           aln_a1, b_reads
#include "host_emu.h"
#include <cstdlib>
static inline unsigned long long __ballot(int p) { return p ? 1ull : 0ull; }
#define __popc __builtin_popcount
#define __popcll __builtin_popcountll
namespace po {
struct Row {
    uint32_t a_idx, b_idx;
    int32_t astart, aend, bstart, bend;
};
}
#include "../phasm_amd/csrc/relevant.hip.h"
using namespace po;

template <class T>
static bool read_n(std::vector<T>& v, size_t n, const char* fmt) {
    v.assign(n + 1, (T)0);
    for (size_t i = 0; i < n; ++i)
        if (scanf(fmt, &v[i]) != 1) return false;
    return true;
}

template <class T>
static void print_n(const std::vector<T>& v, size_t n, const char* fmt) {
    for (size_t i = 0; i < n; ++i) printf(fmt, v[i]);
    printf("\n");
}

// the library's prefix_sum: exclusive offsets and the closing sentinel
static uint32_t scan(const uint32_t* in, uint32_t n, uint32_t* out) {
    uint32_t run = 0;
    for (uint32_t i = 0; i < n; ++i) { out[i] = run; run += in[i]; }
    if (n) out[n] = run;
    return run;
}

int main() {
    uint32_t n_ids, n_rows, n_slots, n_queries;
    if (scanf("%u %u %u %u", &n_ids, &n_rows, &n_slots, &n_queries) != 4) return 1;
    if (2ull * n_rows >= (1ull << 31)) return 1;
    std::vector<uint32_t> len;
    if (!read_n(len, n_ids, "%u")) return 1;
    std::vector<Row> rows(n_rows + 1);
    for (uint32_t i = 0; i < n_rows; ++i)
        if (scanf("%u %u %d %d %d %d", &rows[i].a_idx, &rows[i].b_idx, &rows[i].astart, &rows[i].aend, &rows[i].bstart, &rows[i].bend) != 6) return 1;
    if (!n_slots) n_slots = rr_table_slots(n_rows);
    if (n_slots <= 2ull * n_rows) return 1;   // (a table must have a free slot: the probe loops end at one)
    // ---- run_phase_index ----
    const size_t nn = (size_t)n_ids + 2;
    unsigned long long cnt[16] = {};
    std::vector<unsigned long long> table(n_slots, 0xDEADull);
    std::vector<uint32_t> tval(n_slots, 0xDEADu), deg(nn, 0xDEADu), cur(nn, 0xDEADu), off(nn, 0xDEADu);
    std::fill(deg.begin(), deg.end(), 0u);
    std::fill(cur.begin(), cur.end(), 0u);
    std::fill(off.begin(), off.end(), 0u);
    std::fill(table.begin(), table.end(), RR_EMPTY);
    std::fill(tval.begin(), tval.end(), 0u);
    if (n_rows) LAUNCH(3, 1, k_rr_insert(rows.data(), n_rows, n_ids, table.data(), tval.data(), n_slots, deg.data(), cnt));
    if (n_ids) LAUNCH(3, 1, k_rr_degree(deg.data(), n_ids, cnt));
    const uint32_t total = scan(deg.data(), n_ids, off.data());
    printf("%llu %llu %llu\n", cnt[RX_KEYS], cnt[RX_MAXDEG], cnt[RX_INVALID]);
    if (cnt[RX_INVALID]) return 0;
    if (total != cnt[RX_KEYS] || cnt[RX_KEYS] > 2ull * n_rows) { printf("bound segments\n"); return 0; }
    const uint32_t n_keys = total;
    std::vector<RrEntry> tmp(n_keys + 1, RrEntry{0xDEADu, -7, -7, 0xDEADu}), entries(n_keys + 1, RrEntry{0xDEADu, -7, -7, 0xDEADu});
    std::vector<uint32_t> ex(n_keys + 1, 0xDEADu);
    if (n_keys) {
        LAUNCH(3, 1, k_rr_fill(table.data(), tval.data(), n_slots, rows.data(), n_rows, n_ids, off.data(), cur.data(), tmp.data(), ex.data(), n_keys));
        LAUNCH(3, 1, k_rr_sort(tmp.data(), ex.data(), off.data(), n_keys, n_ids, entries.data()));
        LAUNCH(3, 1, k_rr_place(entries.data(), ex.data(), n_keys, table.data(), tval.data(), n_slots));
    }
    print_n(off, (size_t)n_ids + 1, "%u ");
    for (uint32_t j = 0; j < n_keys; ++j) printf("%u %d %d %u ", entries[j].b, entries[j].a0, entries[j].a1, entries[j].seq);
    printf("\n");
    // ---- run_relevant, once per query; the workspaces go from query to query as they are ----
    const uint32_t W = (n_ids + 31) / 32;
    const size_t Wp = (size_t)W + 1;
    std::vector<uint32_t> bits(6 * Wp, 0xDEADBEEFu), wcnt(3 * Wp, 0xDEADu), wrank(3 * Wp, 0xDEADu);
    for (uint32_t qi = 0; qi < n_queries; ++qi) {
        uint32_t mode, min_span, n_cur, n_pg, n_pa, n_pred;
        if (scanf("%u %u %u %u %u %u", &mode, &min_span, &n_cur, &n_pg, &n_pa, &n_pred) != 6 || mode > 1) return 1;
        std::vector<uint32_t> lc, lpg, lpa, lpred;
        std::vector<int32_t> plen;
        if (!read_n(lc, n_cur, "%u") || !read_n(lpg, n_pg, "%u") || !read_n(lpa, n_pa, "%u") || !read_n(lpred, n_pred, "%u") ||
            !read_n(plen, n_pred, "%d"))
            return 1;
        for (const std::vector<uint32_t>* l : {&lc, &lpg, &lpa, &lpred})
            for (size_t i = 0; i + 1 < l->size(); ++i)
                if ((*l)[i] >= n_ids) return 1;   // (the library refuses it on the host)
        if (!n_cur) {
            printf("0 0 0 0 0 0\n\n\n\n0 \n\n\n\n\n");
            continue;
        }
        uint32_t *ca = bits.data(), *pa = ca + Wp, *gc = ca + 2 * Wp, *gp = ca + 3 * Wp, *rel = ca + 4 * Wp, *g = ca + 5 * Wp;
        unsigned long long c2[16] = {};
        std::fill(bits.begin(), bits.begin() + 4 * Wp, 0u);
        LAUNCH(3, 1, k_rr_mark(lc.data(), n_cur, n_ids, ca));
        LAUNCH(3, 1, k_rr_mark(lc.data(), n_cur, n_ids, gc));
        if (n_pg) LAUNCH(3, 1, k_rr_mark(lpg.data(), n_pg, n_ids, gp));
        if (n_pa) LAUNCH(3, 1, k_rr_mark(lpa.data(), n_pa, n_ids, pa));
        LAUNCH(3, 1, k_rr_mark_seg(lc.data(), n_cur, n_ids, off.data(), entries.data(), n_keys, ca));
        LAUNCH(3, 1, k_rr_count(ca, pa, W, c2));
        const uint64_t n_ca = c2[RG_CA], n_span = c2[RG_SPAN];
        if (n_ca > n_ids || n_span > n_ca) { printf("bound aligning\n"); return 0; }
        const bool fell_back = mode == 0 && n_span < min_span, use_pa = mode == 0 && !fell_back;
        const uint32_t n_rel = (uint32_t)(use_pa ? n_span : n_ca), g_room = fell_back ? n_cur : n_cur + n_pg;
        std::vector<uint32_t> l_ca(n_ca + 1, 0xDEADu), l_rel(n_rel + 1, 0xDEADu), l_b(g_room + 1, 0xDEADu), aln_cnt(n_rel + 2, 0xDEADu),
            aln_off(n_rel + 2, 0xDEADu);
        std::vector<int32_t> om(n_rel + 2, -7);
        std::fill(aln_off.begin(), aln_off.end(), 0u);
        LAUNCH(3, 1, k_rr_select(ca, pa, gc, gp, W, (uint32_t)use_pa, (uint32_t)!fell_back, rel, g, wcnt.data(), wcnt.data() + Wp, wcnt.data() + 2 * Wp));
        uint32_t tot[3];
        for (int k = 0; k < 3; ++k) tot[k] = scan(wcnt.data() + k * Wp, W, wrank.data() + k * Wp);
        LAUNCH(3, 1, k_rr_list(ca, wrank.data(), W, l_ca.data(), (uint32_t)n_ca));
        LAUNCH(3, 1, k_rr_list(rel, wrank.data() + Wp, W, l_rel.data(), n_rel));
        LAUNCH(3, 1, k_rr_list(g, wrank.data() + 2 * Wp, W, l_b.data(), g_room));
        if (n_rel) {
            LAUNCH(3, 1, k_rr_alncount(l_rel.data(), n_rel, n_ids, off.data(), entries.data(), n_keys, g, aln_cnt.data()));
            LAUNCH(3, 1, k_rr_omax(l_rel.data(), n_rel, n_ids, len.data(), lpred.data(), plen.data(), n_pred, table.data(), tval.data(), n_slots,
                                   entries.data(), n_keys, om.data()));
        }
        const uint32_t n_aln = scan(aln_cnt.data(), n_rel, aln_off.data()), n_b = tot[2];
        if (tot[0] != n_ca || tot[1] != n_rel || n_b > g_room || n_aln > n_keys) { printf("bound lists\n"); return 0; }
        std::vector<uint32_t> aln_b(n_aln + 1, 0xDEADu);
        std::vector<int32_t> a0(n_aln + 1, -7), a1(n_aln + 1, -7);
        if (n_aln)
            LAUNCH(3, 1, k_rr_alnwrite(l_rel.data(), n_rel, n_ids, off.data(), entries.data(), n_keys, g, wrank.data() + 2 * Wp, aln_off.data(), n_aln,
                                       aln_b.data(), a0.data(), a1.data()));
        printf("%llu %llu %d %u %u %u\n", (unsigned long long)n_ca, (unsigned long long)n_span, (int)fell_back, n_rel, n_aln, n_b);
        print_n(l_ca, n_ca, "%u ");
        print_n(l_rel, n_rel, "%u ");
        print_n(om, n_rel, "%d ");
        print_n(aln_off, (size_t)n_rel + 1, "%u ");
        print_n(aln_b, n_aln, "%u ");
        print_n(a0, n_aln, "%d ");
        print_n(a1, n_aln, "%d ");
        print_n(l_b, n_b, "%u ");
    }
    return 0;
}
