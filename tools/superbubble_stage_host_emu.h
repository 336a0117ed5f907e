// What superbubbles_host_emu.cpp, bubblechains_host_emu.cpp and cyclic_host_emu.cpp share: the SCC stage and the superbubble stage behind the rank
// prologue of rank_host_emu.h, launched as scc_stage and superbubble_stage (c_api.hip) launch them -- the same memsets, the
// same bounds, the batches and the stop at the first round that changes nothing from round_phase of components.hip.h.
// Included after superbubbles.hip.h, `using namespace po` and rank_host_emu.h.  The workspaces start as a call before could
// have left them.
#pragma once

struct Batches {
    unsigned long long rcnt[CC_BATCH];
    uint64_t words[CC_BATCH];
    uint32_t max_batch = 0, in_batch = 0, batches = 0;
    bool begin(uint32_t batch) {
        if (batch == 0 || batch > CC_BATCH) return false;
        std::memset(rcnt, 0, sizeof rcnt);
        max_batch = std::max(max_batch, batch);
        in_batch = 0;
        return true;
    }
    bool end(uint32_t batch, const volatile uint64_t*& out) {
        if (in_batch != batch) return false;   // (every round of the batch was launched, and no more)
        for (uint32_t j = 0; j < CC_BATCH; ++j) words[j] = j < batch ? rcnt[j] : 0xDEADu;
        out = words;
        return true;
    }
    void note(uint32_t j) {
        if (j != in_batch) in_batch = CC_BATCH + 1;
        ++in_batch;
    }
};

struct SccEmu : Batches {
    uint32_t n, n_order;
    const EdgeRanks* ends;
    uint8_t *live, *mark, *has_in, *has_out;
    uint32_t *scc, *colour;
    void trim_round(uint32_t j) {
        note(j);
        if (n) LAUNCH(3, 4, k_scc_trim_edges(ends, n, n_order, live, has_in, has_out));
        LAUNCH(3, 4, k_scc_trim_ranks(n_order, live, scc, has_in, has_out, rcnt + j));
    }
    void colour_init() { LAUNCH(3, 4, k_scc_colour_init(n_order, live, colour, mark)); }
    void forward_round(uint32_t j) {
        note(j);
        if (n) LAUNCH(3, 4, k_scc_forward(ends, n, n_order, live, colour, rcnt + j));
    }
    void back_init() { LAUNCH(3, 4, k_scc_back_init(n_order, live, colour, mark)); }
    void backward_round(uint32_t j) {
        note(j);
        if (n) LAUNCH(3, 4, k_scc_backward(ends, n, n_order, live, colour, mark, rcnt + j));
    }
    bool retire(uint64_t& retired) {
        unsigned long long c = 0;
        LAUNCH(3, 4, k_scc_retire(n_order, live, colour, mark, scc, &c));
        retired = c;
        return true;
    }
};

static void scan(const std::vector<uint32_t>& in, uint32_t n, std::vector<uint32_t>& out, uint64_t& total) {   // the library's prefix_sum
    total = 0;
    for (uint32_t r = 0; r < n; ++r) { out[r] = (uint32_t)total; total += in[r]; }
}

// Everything the stage leaves behind, for the caller to print or to go on with.
struct SuperbubbleStage {
    std::vector<uint32_t> scc, node_scc, flagw, w, cin, cout, off_in, off_out, cur_in, cur_out, list_in, list_out, lvl_f, lvl_b, idom, ipdom,
        depth, exit_of, encl, inside, total, d_exit, d_inside;
    std::vector<uint8_t> live, mark, has_in, has_out, pflags, eclass, dead, d_flags;
    std::vector<Scc> sccs;
    std::vector<Bubble> table;
    unsigned long long cnt[16] = {};
    Batches ops;
    uint32_t n_scc = 0, n_bubbles = 0, level_rounds = 0, discard_rounds = 0;
    uint64_t n_real = 0, n_dedges = 0, levels_f = 0, levels_b = 0, beyond = 0, per_level = 0;

    // false: a bound was reached and "bound WHAT" is on stdout.  With an empty order only the SCC stage runs.
    bool run(RankedInput& g, std::vector<uint32_t>& colour) {
        if (!scc_rounds(g, colour)) return false;
        return !g.n_order || dag(g, [] { return false; });
    }
    // the two halves, as scc_rounds and superbubble_dag (c_api.hip) launch them; cyclic_host_emu.cpp runs them on flat graphs.
    // seed() may mark bubbles dead before the discard rounds (true: it did something, so the rounds run)
    bool scc_rounds(RankedInput& g, std::vector<uint32_t>& colour);
    template <class Seed> bool dag(RankedInput& g, Seed&& seed);
};

inline bool SuperbubbleStage::scc_rounds(RankedInput& g, std::vector<uint32_t>& colour) {
    const uint32_t n = g.n, n_order = g.n_order, nn = g.nn;
    const std::vector<EdgeRanks>& ends = g.ends;
    // ---- the SCC stage, as scc_stage launches it
    for (auto* v : {&scc, &node_scc, &flagw}) v->assign(nn, 0xDEADu);
    for (auto* v : {&live, &mark, &has_in, &has_out, &pflags}) v->assign(nn, 9);
    eclass.assign(n + 1, 9);
    sccs.assign(nn, Scc{0xDEADu, 0xDEADu, 0xDEADull, 0xDEADu, 0xDEADu});
    SccWork W;
    if (n_order) {
        SccEmu sops;
        sops.n = n; sops.n_order = n_order; sops.ends = ends.data(); sops.live = live.data(); sops.mark = mark.data();
        sops.has_in = has_in.data(); sops.has_out = has_out.data(); sops.scc = scc.data(); sops.colour = colour.data();
        LAUNCH(3, 4, k_scc_init(n_order, live.data(), scc.data(), has_in.data(), has_out.data()));
        if (scc_drive(sops, n_order, W) != SCC_DONE) { printf("bound scc\n"); return false; }
        LAUNCH(3, 4, k_scc_roots(scc.data(), n_order, g.root.data(), flagw.data()));
    }
    n_scc = number_roots(g);
    if (n_scc) {
        std::memset(sccs.data(), 0, (size_t)n_scc * sizeof(Scc));
        LAUNCH(3, 4, k_scc_label_nodes(scc.data(), g.index.data(), g.val.data(), n_order, n_scc, node_scc.data(), sccs.data()));
        if (n) LAUNCH(3, 4, k_scc_edges(ends.data(), n, n_order, n_scc, node_scc.data(), sccs.data(), eclass.data(), flagw.data(), g.cnt));
        LAUNCH(3, 4, k_scc_flags(n_order, n_scc, node_scc.data(), flagw.data(), sccs.data(), pflags.data()));
        LAUNCH(3, 4, k_scc_max(sccs.data(), n_scc, g.cnt));
    }
    return true;
}

template <class Seed>
inline bool SuperbubbleStage::dag(RankedInput& g, Seed&& seed) {
    const uint32_t n = g.n, n_order = g.n_order, nn = g.nn;
    const std::vector<EdgeRanks>& ends = g.ends;
    // ---- the superbubbles, as run_superbubbles launches them
    for (auto* v : {&w, &cin, &cout, &off_in, &off_out, &cur_in, &cur_out, &lvl_f, &lvl_b, &idom, &ipdom, &depth, &exit_of, &encl, &inside, &total,
                    &d_exit, &d_inside})
        v->assign(nn, 0xDEADu);
    for (auto* v : {&list_in, &list_out}) v->assign(n + 1, 0xDEADu);
    for (auto* v : {&dead, &d_flags}) v->assign(nn, 9);
    table.assign(nn, Bubble{0xDEADu, 0xDEADu, 0xDEADu, 0xDEADu});
    LAUNCH(3, 4, k_sb_init(n_order, n_scc, node_scc.data(), sccs.data(), w.data(), cin.data(), cout.data(), idom.data(), ipdom.data(),
                           depth.data(), exit_of.data(), encl.data(), total.data(), dead.data()));
    if (n) LAUNCH(3, 4, k_sb_degrees(ends.data(), n, n_order, eclass.data(), w.data(), cin.data(), cout.data(), cnt));
    uint64_t sum_in = 0, sum_out = 0;
    scan(cin, n_order, off_in, sum_in);
    scan(cout, n_order, off_out, sum_out);
    std::fill(cur_in.begin(), cur_in.begin() + n_order, 0u);
    std::fill(cur_out.begin(), cur_out.begin() + n_order, 0u);
    if (n)
        LAUNCH(3, 4, k_sb_fill(ends.data(), n, n_order, eclass.data(), cin.data(), cout.data(), off_in.data(), off_out.data(), cur_in.data(),
                               cur_out.data(), list_in.data(), list_out.data()));
    LAUNCH(3, 4, k_sb_nodes(n_order, pflags.data(), cin.data(), cout.data(), w.data(), lvl_f.data(), lvl_b.data(), cnt));
    n_real = cnt[BC_REAL];
    n_dedges = cnt[BC_DEDGES];
    if (sum_in != n_dedges || sum_out != n_dedges || n_dedges > n || n_real > n_order) { printf("bound degrees\n"); return false; }
    uint64_t ignored = 0;
    int how = round_phase(ops, n_real, [&](uint32_t j) {
        ops.note(j);
        if (n) LAUNCH(3, 4, k_sb_level(ends.data(), n, n_order, eclass.data(), lvl_f.data(), lvl_b.data(), ops.rcnt + j));
    }, level_rounds, ops.batches, ignored);
    if (how != ROUNDS_DONE) { printf("bound levels\n"); return false; }
    if (level_rounds > n_real) beyond = level_rounds - n_real;
    LAUNCH(3, 4, k_sb_level_max(n_order, lvl_f.data(), lvl_b.data(), cnt));
    levels_f = cnt[BC_LEVF];
    levels_b = cnt[BC_LEVB];
    if (levels_f > n_real || levels_b > n_real) { printf("bound level count\n"); return false; }
    for (uint32_t l = 1; l <= levels_f; ++l, ++per_level)
        LAUNCH(3, 4, k_sb_tree(n_order, n, l, lvl_f.data(), off_in.data(), cin.data(), list_in.data(), w.data(), (uint32_t)SBW_SOURCE, idom.data(),
                               depth.data(), cnt));
    for (uint32_t l = 1; l <= levels_b; ++l, ++per_level)
        LAUNCH(3, 4, k_sb_tree(n_order, n, l, lvl_b.data(), off_out.data(), cout.data(), list_out.data(), w.data(), (uint32_t)SBW_SINK, ipdom.data(),
                               depth.data(), cnt));
    LAUNCH(3, 4, k_sb_pairs(n_order, w.data(), idom.data(), ipdom.data(), exit_of.data()));
    for (uint32_t l = 1; l <= levels_f; ++l, ++per_level)
        LAUNCH(3, 4, k_sb_encl(n_order, l, lvl_f.data(), idom.data(), exit_of.data(), encl.data()));
    const bool seeded = seed();
    if (cnt[BC_LOOPS]) LAUNCH(3, 4, k_sb_dead_init(n_order, w.data(), idom.data(), exit_of.data(), encl.data(), dead.data()));
    if (cnt[BC_LOOPS] || seeded) {
        how = round_phase(ops, n_real, [&](uint32_t j) {
            ops.note(j);
            LAUNCH(3, 4, k_sb_dead_round(n_order, exit_of.data(), encl.data(), dead.data(), ops.rcnt + j));
        }, discard_rounds, ops.batches, ignored);
        if (how != ROUNDS_DONE) { printf("bound discards\n"); return false; }
        if (discard_rounds > n_real) beyond = std::max<uint64_t>(beyond, discard_rounds - n_real);
    }
    LAUNCH(3, 4, k_sb_label(n_order, g.val.data(), w.data(), idom.data(), exit_of.data(), encl.data(), dead.data(), inside.data(), total.data(),
                            g.root.data(), d_exit.data(), d_inside.data(), d_flags.data(), cnt));
    n_bubbles = number_roots(g);
    if (cnt[BC_WALK]) { printf("bound walk\n"); return false; }
    if (n_bubbles > n_real || cnt[BC_NESTED] > n_bubbles) { printf("bound bubbles\n"); return false; }
    if (cnt[BC_NESTED])
        for (uint32_t l = (uint32_t)levels_f; l >= 1; --l, ++per_level)
            LAUNCH(3, 4, k_sb_sum(n_order, l, lvl_f.data(), g.root.data(), inside.data(), total.data()));
    if (n_bubbles)
        LAUNCH(3, 4, k_sb_table(n_order, n_bubbles, g.val.data(), g.root.data(), g.index.data(), exit_of.data(), inside.data(), total.data(),
                                table.data()));
    return true;
}
