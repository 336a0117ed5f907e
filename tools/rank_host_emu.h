// What components_host_emu.cpp and partition_host_emu.cpp share: their input and the rank prologue, launched as ranked_open
// (c_api.hip) launches it.  Included after components.hip.h and `using namespace po`.  The workspaces start as a call before
// could have left them -- on a handle the two stages take turns in the same ones.
#pragma once

struct RankedInput {
    uint32_t n_total = 0, n = 0, n_order = 0, pad = 0, nn = 0;
    std::vector<Edge> e;
    std::vector<uint32_t> val, index;
    std::vector<uint8_t> root;
    std::vector<EdgeRanks> ends;
    unsigned long long cnt[16] = {};
};

// stdin: n_total n_edges n_order, one "u v" line per edge ("u v weight" with `weights`), the nodes in node order.  The
// identity words go to `ident`.  Returns -1 to go on, else the exit status ("invalid N" or "order" is on stdout then).
static int ranked_input(RankedInput& g, std::vector<uint32_t>& ident, bool weights = false) {
    uint32_t n_order_in;
    if (scanf("%u %u %u", &g.n_total, &g.n, &n_order_in) != 3) return 1;
    const uint32_t n_total = g.n_total, n = g.n;
    g.e.resize(n + 1);
    for (uint32_t i = 0; i < n; ++i) {
        if (scanf("%u %u", &g.e[i].u, &g.e[i].v) != 2) return 1;
        g.e[i].weight = 100;
        if (weights && scanf("%d", &g.e[i].weight) != 1) return 1;
        g.e[i].overlap_len = 17;
    }
    std::vector<unsigned long long> nrank(n_total + 1, NODE_NO_RANK);
    for (uint32_t i = 0; i < n_order_in; ++i) { uint32_t x; if (scanf("%u", &x) != 1 || x >= n_total) return 1; nrank[x] = ((unsigned long long)(3u * i + 5) << 2) | (i & 3); }
    const uint32_t pad = g.pad = merge_sort_pad(n_total), nn = g.nn = n_total + 2;
    std::vector<unsigned long long> key(pad, 7);
    std::vector<uint32_t> rank_of(nn, 0xFFFFFFFFu);
    g.val.assign(pad, 0xDEADu);
    g.index.assign(nn, 0xDEADu);
    ident.assign(nn, 0xDEADu);
    g.root.assign(nn, 9);
    g.ends.assign(n + 1, EdgeRanks{0xDEADu, 0xDEADu});
    LAUNCH((pad + 3) / 4, 4, k_cc_keys(nrank.data(), n_total, pad, key.data(), g.val.data()));
    merge_sort_steps(n_total, [&](uint32_t j, uint32_t k) { LAUNCH((pad + 3) / 4, 4, k_merge_bitonic(key.data(), g.val.data(), pad, j, k)); });
    LAUNCH((pad + 3) / 4, 4, k_cc_init(key.data(), g.val.data(), pad, n_total, ident.data(), rank_of.data(), g.cnt));
    if (n) LAUNCH(3, 4, k_cc_ends(g.e.data(), n, n_total, rank_of.data(), g.ends.data(), g.cnt));
    if (g.cnt[KC_INVALID]) { printf("invalid %llu\n", g.cnt[KC_INVALID]); return 0; }
    if (g.cnt[KC_ORDER] != n_order_in) { printf("order\n"); return 0; }
    g.n_order = (uint32_t)g.cnt[KC_ORDER];
    return -1;
}

// the prefix_sum of the library over the root bytes: index[r] = roots below r; returns their number
static uint32_t number_roots(RankedInput& g) {
    uint32_t n_roots = 0;
    for (uint32_t r = 0; r < g.n_order; ++r) { g.index[r] = n_roots; n_roots += g.root[r]; }
    return n_roots;
}
