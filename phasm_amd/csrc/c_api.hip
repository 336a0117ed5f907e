// Host side of libphasm_overlap.so: the C ABI declared in include/phasm_overlap.h.
// Holds the read set (2-bit or 8-bit packed 64-bit words), keeps a device-resident copy, and
// drives the kernels of kernels.hip.h on the handle's own HIP stream.  No CPU compute path.
#include "../../include/phasm_overlap.h"

#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <execinfo.h>
#include <fcntl.h>
#include <signal.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <system_error>
#include <thread>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "kernels.hip.h"
#include "extend.hip.h"
#include "layout.hip.h"
#include "reduce.hip.h"
#include "tips.hip.h"
#include "diamond.hip.h"
#include "merge.hip.h"
#include "coverage.hip.h"
#include "components.hip.h"
#include "partition.hip.h"
#include "superbubbles.hip.h"
#include "cyclic.hip.h"
#include "bubblechains.hip.h"
#include "ringchains.hip.h"
#include "contigs.hip.h"
#include "phase.hip.h"
#include "relevant.hip.h"
#include "spell.hip.h"
#include "paths.hip.h"
#include "walk.hip.h"
#include "resident.hip.h"
#include "large.hip.h"

namespace {

// workspaces of po_layout_reduce (po_handle::d_red, reduce.hip.h)
enum { RB_CNT, RB_DEG, RB_OFF, RB_CUR, RB_TKEY, RB_TTGT, RB_TEID, RB_CTGT, RB_CW, RB_CEID, RB_CIDPOS, RB_STGT, RB_SEID, RB_STATE,
       RB_FLAG1, RB_FLAGS, RB_KEEP, RB_KOFF, RB_N };
// workspaces of po_layout_tips (po_handle::d_tip)
enum { TB_CNT, TB_OUTDEG, TB_OUTSUM, TB_INDEG, TB_INSUM, TB_MARK, TB_CAND, TB_CSTATE, TB_EFLAG, TB_FLAGS, TB_KEEP, TB_KOFF,
       TB_TKEY, TB_TVAL, TB_ALIVE, TB_RCNT, TB_N };
// workspaces of po_layout_merge (merge.hip.h)
enum { MB_CNT, MB_RCNT, MB_OUTDEG, MB_INDEG, MB_OUTE, MB_INE, MB_LINK, MB_BACK, MB_JB0, MB_JB1, MB_HOPS0, MB_HOPS1, MB_WS0, MB_WS1,
       MB_HKEY, MB_HVAL, MB_HLEN, MB_HSUM, MB_PATHK, MB_LENS, MB_PSUM, MB_NPATH, MB_NPOS, MB_EFLAG, MB_KEEP, MB_KOFF, MB_TMP, MB_LEN,
       MB_N };
// workspaces of po_layout_coverage (coverage.hip.h)
enum { VB_CNT, VB_USED, VB_NODEOF, VB_LEN, VB_TABLE, VB_SUM, VB_SETCNT, VB_OFF, VB_CUR, VB_LIST, VB_OUT, VB_N };
// what every analysis stage on a graph result works in (po_handle::d_rank, ranked_open): counters, change words, the sort,
// node -> rank, the two ranks of every edge, the root bytes and their prefix sum
enum { RK_CNT, RK_RCNT, RK_KEY, RK_VAL, RK_RANKOF, RK_ENDS, RK_ROOT, RK_INDEX, RK_N };
// workspaces of po_layout_components (components.hip.h) beyond those
enum { KB_P, KB_COMP, KB_ECOMP, KB_TABLE, KB_N };
// workspaces of po_layout_partition (partition.hip.h) beyond those
enum { PB_LIVE, PB_SCC, PB_COLOUR, PB_MARK, PB_HASIN, PB_HASOUT, PB_NODESCC, PB_FLAGW, PB_FLAGS, PB_ECLASS, PB_TABLE, PB_N };
// workspaces of po_layout_superbubbles (superbubbles.hip.h) beyond those of the rank scaffold and of po_layout_partition
enum { UB_CNT, UB_W, UB_CIN, UB_COUT, UB_OFFIN, UB_OFFOUT, UB_CURIN, UB_CUROUT, UB_LISTIN, UB_LISTOUT, UB_LVLF, UB_LVLB, UB_IDOM, UB_IPDOM,
       UB_DEPTH, UB_EXIT, UB_ENCL, UB_INSIDE, UB_TOTAL, UB_DEAD, UB_EXITOUT, UB_INSIDEOUT, UB_FLAGSOUT, UB_TABLE, UB_N };
// workspaces of po_layout_superbubbles_all (cyclic.hip.h) beyond those of the rank scaffold, po_layout_partition and
// po_layout_superbubbles, all three for twice the ranks: counters; per rank the split byte and its prefix sum, the root a run
// gives a rootless SCC, the SCC of the graph itself, the bytes "in a non-singleton SCC" / "lowest rank of a rootless SCC" /
// "not certified" / "root of the cycle search" / "(s, t) with an edge t -> s" / "has a self-loop", the merged pairs, holders,
// sizes, totals and bytes, the four words of the cycle search; per flat rank its node and its original rank; per SCC of the
// flat graph the three lowest ranks; the flat edge list
enum { YB_CNT, YB_SPLIT, YB_SIDX, YB_ROOTOF, YB_SCC0, YB_CYCLIC0, YB_ROOTLESS, YB_UNCERTAIN, YB_ISROOT, YB_FILTERED, YB_LOOP, YB_MEXIT,
       YB_MINSIDE, YB_MSIZE, YB_MTOTAL, YB_MISEXIT, YB_MFILTERED, YB_MROOT, YB_DIST, YB_PAR, YB_DIN, YB_PIN, YB_NODE, YB_ORIG, YB_BESTIN,
       YB_BESTOUT, YB_BESTLOW, YB_FLAT, YB_N };
// workspaces of po_layout_bubblechains (bubblechains.hip.h) beyond those of the rank scaffold, po_layout_partition and
// po_layout_superbubbles; the last four are the two buffer pairs of the ring election (ringchains.hip.h), which only
// po_layout_bubblechains_all and po_layout_contigs_all take
enum { HB_CNT, HB_FW, HB_NEXT, HB_PRED, HB_TOP, HB_JB0, HB_JB1, HB_HOPS0, HB_HOPS1, HB_NHEAD, HB_NPOS, HB_CB, HB_CN, HB_LAST, HB_CE,
       HB_CHAINOUT, HB_BUBBLEOUT, HB_EDGEOUT, HB_TABLE, HB_RPTR0, HB_RPTR1, HB_RMN0, HB_RMN1, HB_N };
// workspaces of po_layout_contigs (contigs.hip.h) beyond those of the rank scaffold and, without an exclude set from the caller,
// of the three stages that po_layout_bubblechains runs
enum { CB_CNT, CB_EXCL, CB_LEN, CB_INDEG, CB_OUTDEG, CB_INE, CB_NLEN, CB_CLS, CB_JB0, CB_JB1, CB_HOPS0, CB_HOPS1, CB_WS0, CB_WS1, CB_CJ0,
       CB_CJ1, CB_OK0, CB_OK1, CB_HEADOF, CB_PN, CB_PLAST, CB_PLEN, CB_KEPT, CB_KEY, CB_VAL, CB_CONTIGOUT, CB_POSOUT, CB_TABLE, CB_N };
// workspaces of po_phase_branch (phase.hip.h): counters (the greatest key behind them), the level histogram, the levels, the inputs,
// bitsets and intervals of the read sets and of the paths, the table, rl / keep byte / place per extension id, the kept list,
// keep byte / place per kept entry, the survivors
enum { FB_CNT, FB_HIST, FB_LEVELS, FB_OM, FB_ALNOFF, FB_ALNB, FB_A0, FB_A1, FB_POFF, FB_PIDS, FB_SOFF, FB_SIDS, FB_SBITS, FB_PBITS, FB_SIV,
       FB_PIV, FB_TABLE, FB_RL, FB_KEEP, FB_PLACE, FB_KCAND, FB_KEXT, FB_KRL, FB_KEEP2, FB_PLACE2, FB_SCAND, FB_SEXT, FB_SRL, FB_N };
// workspaces of po_phase_index and po_phase_relevant (relevant.hip.h).  The index: counters, keys per read, fill cursors, the
// unsorted entries and their x.  The gather: the uploaded lists, the six bitsets, the three popcounts and ranks per word, the
// three lists, count / offset / overlap_max per relevant read, the alignments
enum { XB_CNT, XB_DEG, XB_CUR, XB_TMP, XB_EX, XB_LISTS, XB_BITS, XB_WCNT, XB_WRANK, XB_CA, XB_REL, XB_B, XB_ALNCNT, XB_ALNOFF, XB_OM,
       XB_ALNB, XB_A0, XB_A1, XB_N };
// workspaces of po_spell (spell.hip.h): the uploaded input (seq_off, piece_read, piece_take behind one another), the 32-bit scan
// of the takes, the 64-bit offsets of the pieces and of the sequences
enum { SB_IN, SB_SCAN, SB_POFF, SB_SOFF, SB_N };
// workspaces of po_phase_paths (paths.hip.h) beyond those of the rank scaffold and of the three stages that
// po_layout_bubblechains runs: counters, bubbles per chain and their offsets, home / bubble number / done word / count per rank,
// entrance per bubble, the two sorted key arrays of the edges, first and last place of every tail and of every head, the three
// counts per bubble, the length of every listed path
enum { QB_CNT, QB_NB, QB_COFF, QB_HOME, QB_BIDX, QB_BENT, QB_DONE, QB_COUNT, QB_KEYOUT, QB_KEYIN, QB_OFIRST, QB_OLAST, QB_IFIRST, QB_ILAST,
       QB_NLIST, QB_NPRED, QB_NIN, QB_PLEN, QB_N };
// what a po_phase_paths result holds in HBM (po_result::d_pp): the table, the three CSR pairs, the offsets of the paths
enum { PR_TABLE, PR_INOFF, PR_INNODES, PR_PREDOFF, PR_PREDNODE, PR_PREDW, PR_BPO, PR_POFF, PR_PATHS, PR_N };
// workspaces of po_phase_large (large.hip.h): counters, the uploaded inputs, the bitsets and intervals of the interior nodes,
// the slot of every node of the graph, the score of every listed path of the bubble
enum { LB_CNT, LB_OM, LB_ALNOFF, LB_ALNB, LB_A0, LB_A1, LB_NOFF, LB_NIDS, LB_NBITS, LB_NIV, LB_SLOT, LB_SCORE, LB_N };
// events of the layout calls: one count for the handle and for the kit that carries them from a closed handle to the next
constexpr int EV_LAY_N = 143;
// the first event of each call's slice of po_handle::ev_lay (a slice ends where the next begins)
enum { EV_EDGES = 0, EV_REDUCE = 4, EV_TIPS = 9, EV_NODE_ORDER = 15, EV_DIAMONDS = 18, EV_MERGE = 22, EV_COVERAGE = 27, EV_COMPONENTS = 30,
       EV_PARTITION = 34, EV_SUPERBUBBLES = 38, EV_BUBBLECHAINS = 45, EV_CONTIGS = 54, EV_PHASE = 67, EV_PHASE_INDEX = 73,
       EV_RELEVANT = 77, EV_SPELL = 81, EV_PATHS = 83, EV_WALK = 94, EV_CYCLIC = 96, EV_CHAINS_ALL = 106, EV_CONTIGS_ALL = 118, EV_LARGE = 134, EV_RESIDENT = 138 };
static_assert(EV_BUBBLECHAINS + 9 == EV_CONTIGS, "po_layout_bubblechains has nine events");
static_assert(EV_CONTIGS + 13 == EV_PHASE, "po_layout_contigs has thirteen events");
static_assert(EV_PHASE + 6 == EV_PHASE_INDEX, "po_phase_branch has six events");
static_assert(EV_PHASE_INDEX + 4 == EV_RELEVANT, "po_phase_index has four events");
static_assert(EV_RELEVANT + 4 == EV_SPELL, "po_phase_relevant has four events");
static_assert(EV_SPELL + 2 == EV_PATHS, "po_spell has two events");
static_assert(EV_PATHS + 11 == EV_WALK, "po_phase_paths has eleven events");
static_assert(EV_WALK + 2 == EV_CYCLIC, "po_walk_step has two events");
static_assert(EV_CYCLIC + 10 == EV_CHAINS_ALL, "po_layout_superbubbles_all has ten events");
static_assert(EV_CHAINS_ALL + 12 == EV_CONTIGS_ALL, "po_layout_bubblechains_all has twelve events: those ten and two of its own");
static_assert(EV_CONTIGS_ALL + 16 == EV_LARGE, "po_layout_contigs_all has sixteen events");
static_assert(EV_LARGE + 4 == EV_RESIDENT, "po_phase_large has four events");
static_assert(EV_RESIDENT + 5 == EV_LAY_N, "the five events of po_walk_step_resident are the last of the layout events");
constexpr int TIP_BATCH = 24;   // rounds of po_layout_tips per readback (words [32..55] of the landing zone)

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    bool arena = false;   // carved out of the handle's arena (po_handle::arena_*): lives until the handle dies
    template <typename T> T* as() const { return static_cast<T*>(p); }
    void release() {
        if (p && !arena) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        arena = false;
    }
};

// Every range of HOST memory this library makes visible to the GPU (hipHostMalloc, hipHostRegister) is noted here, for
// the whole life of the process: po_debug_host_ranges hands the list out, and the tests assert that no page of the reads
// they handed to po_add_sequence ever lay inside one (the library's device->host copies and
// host-mapped stores can only reach memory that is on this list).
struct PinNote {
    uint64_t base, bytes;
    uint32_t kind;   // 1 hipHostMalloc, 2 hipHostRegister (packed read store), bit 8: still live
};
std::mutex g_pin_mu;
std::vector<PinNote> g_pins;
uint64_t g_pins_ever = 0;
constexpr size_t PIN_LOG_MAX = 1u << 16;
void pin_note(const void* p, size_t bytes, uint32_t kind) {
    if (!p) return;
    std::lock_guard<std::mutex> lock(g_pin_mu);
    ++g_pins_ever;
    for (PinNote& n : g_pins)   // (the same range again: one entry)
        if (n.base == (uint64_t)(uintptr_t)p && n.bytes == bytes && (n.kind & 0xFFu) == kind) {
            n.kind |= 0x100u;
            return;
        }
    if (g_pins.size() < PIN_LOG_MAX) g_pins.push_back(PinNote{(uint64_t)(uintptr_t)p, (uint64_t)bytes, kind | 0x100u});
}
void pin_drop(const void* p) {
    if (!p) return;
    std::lock_guard<std::mutex> lock(g_pin_mu);
    for (PinNote& n : g_pins)
        if (n.base == (uint64_t)(uintptr_t)p && (n.kind & 0x100u)) n.kind &= ~0x100u;
}

// host-pinned buffer (hipHostMalloc): every device->host copy of this library lands in one of these, never in
// pageable heap memory -- the HIP runtime then neither stages the copy nor pins (and caches the pin of) a range
// of the caller's malloc heap
struct HostBuf {
    void* p = nullptr;
    size_t cap = 0;
    void release() {
        if (p) {
            pin_drop(p);
            (void)hipHostFree(p);
        }
        p = nullptr;
        cap = 0;
    }
};

// Stage-boundary timing events (po_stats.ms_index .. ms_emit).  A recorded event is a marker the command processor has to
// retire between two kernels (~5 us each, measured): a whole-set call records all of them, the pieces of a streamed step only
// the pairs around the two big kernels (ms_scan_probe, ms_verify_kernel) unless PHASM_PHASE_EVENTS=1 / PHASM_STREAM_TRACE ask.
inline int phase_events_env() {
    // -1: default (whole-set calls record every stage boundary, the pieces of a streamed step NOTHING but their end -- round 4:
    // with the rows going home as records the step is paced by the device, and seven markers per piece were 35 us of it);
    // 0: nothing but the end anywhere; 1: every boundary everywhere; 2: pieces record the pairs around their two big kernels
    // (ms_scan_probe, ms_verify_kernel) and their start / end (ms_total) -- what bench.py's extra steps ask for
    if (const char* e = getenv("PHASM_PHASE_EVENTS")) {
        const int v = atoi(e);
        return v == 1 ? 1 : v == 2 ? 2 : 0;
    }
    return getenv("PHASM_STREAM_TRACE") ? 1 : -1;
}
enum { EV_START = 0, EV_INDEX, EV_COUNT, EV_FILL, EV_VERIFY, EV_SELECT, EV_EMIT, EV_PROBE0, EV_PROBE1, EV_VER0, EV_VER1, EV_DONE, EV_N };

}  // namespace

constexpr int PO_MAX_PIECES = 16;

// The packed host stores live in memory that is REGISTERED with the HIP runtime from the moment it is allocated
// (page-aligned malloc + hipHostRegister, portable across devices): po_add_sequence grows the stores, so the cost of
// pinning is paid there, piece by piece as the vector doubles -- not inside the first po_overlaps call, whose H2D then
// runs at the DMA rate straight away (a cold call used to start with 2-4 ms of hipHostRegister).  Without a GPU (or
// with PHASM_NO_PIN) the registration fails or is skipped and the memory is plain heap: the copy works either way.
struct RegHeader {
    size_t bytes;
    int registered;
};
constexpr size_t REG_PAGE = 4096;
thread_local bool g_reg_defer = false;   // (see RegAlloc::reg_now)
template <class T>
struct RegAlloc {
    using value_type = T;
    RegAlloc() = default;
    template <class U> RegAlloc(const RegAlloc<U>&) {}
    T* allocate(size_t n) {
        const size_t bytes = ((n * sizeof(T) + REG_PAGE - 1) / REG_PAGE) * REG_PAGE;
        void* base = nullptr;
        if (posix_memalign(&base, REG_PAGE, bytes + REG_PAGE) != 0 || !base) throw std::bad_alloc();
        RegHeader* hd = static_cast<RegHeader*>(base);
        hd->bytes = bytes;
        hd->registered = 0;
        char* data = static_cast<char*>(base) + REG_PAGE;
        if (getenv("PHASM_POISON_HOST")) std::memset(data, 0xA5, bytes);   // (tests: a word nobody wrote shows)
        if (!g_reg_defer) reg_now(data);
        return reinterpret_cast<T*>(data);
    }
    // page-lock the block behind `data` (allocate() does it at once, unless the caller has asked to do it later: po_add_fasta
    // registers the stores on a thread of its own WHILE the packing threads fill them -- the call blocks until the runtime is
    // up and pins 4 KB pages one by one, 40-60 ms per 190 MB store, which used to sit in front of the packing)
    static void reg_now(void* data) {
        RegHeader* hd = reinterpret_cast<RegHeader*>(static_cast<char*>(data) - REG_PAGE);
        if (hd->registered || hd->bytes < (1u << 20) || getenv("PHASM_NO_PIN")) return;
        if (hipHostRegister(data, hd->bytes, hipHostRegisterPortable) == hipSuccess) {
            hd->registered = 1;
            pin_note(data, hd->bytes, 2u);
        } else {
            (void)hipGetLastError();
        }
    }
    // vector::resize(n) (no value) leaves the new words as they are: the caller writes every one of them
    template <class U> void construct(U*) noexcept {}
    template <class U, class A0, class... Args> void construct(U* q, A0&& a0, Args&&... args) {
        ::new (static_cast<void*>(q)) U(std::forward<A0>(a0), std::forward<Args>(args)...);
    }
    void deallocate(T* p, size_t) {
        char* base = reinterpret_cast<char*>(p) - REG_PAGE;
        RegHeader* hd = reinterpret_cast<RegHeader*>(base);
        if (hd->registered) {
            pin_drop(p);
            (void)hipHostUnregister(p);
        }
        free(base);
    }
    template <class U> bool operator==(const RegAlloc<U>&) const { return true; }
    template <class U> bool operator!=(const RegAlloc<U>&) const { return false; }
};
using WordStore = std::vector<uint64_t, RegAlloc<uint64_t>>;
inline bool store_is_pinned(const WordStore& w) {
    if (w.capacity() == 0) return false;
    const RegHeader* hd = reinterpret_cast<const RegHeader*>(reinterpret_cast<const char*>(w.data()) - REG_PAGE);
    return hd->registered != 0;
}
constexpr size_t STAGE_MAX = 4u << 20;   // larger sources are registered stores (or, failing that, go as they are)

struct po_handle {
    int device = 0;
    bool dev_ready = false;
    hipStream_t stream = nullptr;
    hipEvent_t ev_sets[2][EV_N] = {};   // (two sets: the pieces of a streamed step alternate, a piece's stage times are read one piece later)
    hipEvent_t* ev = ev_sets[0];
    hipEvent_t ev_up0 = nullptr, ev_up1 = nullptr;
    uint64_t* pinned = nullptr;  // host-pinned landing zone for device totals/counters (128 x u64; [64..95]: the two zones of a streamed step's pieces)
    uint64_t* pinned_dev = nullptr;  // the same memory as the device sees it (kernels write totals there directly)
    int n_cu = 256;
    size_t lds_max = 64 * 1024;
    std::string err;

    // host read store
    int bits = 2;
    std::vector<std::string> ids;
    std::vector<uint32_t> len;
    std::vector<uint64_t> cum_len;   // running sum of len (shard_range), extended as reads are added
    // Packed reads live in TWO host stores: words[0] holds the reads with an even index, words[1] those with an odd
    // index, woff[r] is read r's first word inside ITS store.  `phasm overlap` adds every read as (x, revcomp x):
    // when every odd read is exactly the reverse complement of its even partner (all_pairs_rc, checked word by word
    // as the reads arrive) only store 0 crosses PCIe and store 1 is rebuilt on the device -- half the H2D bytes.
    // On the device the two stores are one buffer [store 0 | store 1 | padding]; d_woff holds absolute offsets.
    std::vector<uint64_t> woff;
    WordStore words[2];
    bool all_pairs_rc = true;   // every complete (even, odd) pair so far: same length, odd == revcomp(even), no exception records
    bool all_pairs_rcx = true;  // the same with exception records allowed: such a pair was compared byte by byte on the host (pair_state 1)
    uint64_t base1 = 0;         // first word of store 1 in the device buffer (set at upload)
    uint64_t dev_words = 0;     // words in the device buffer, padding included
    uint64_t upload_bytes = 0;  // bytes the last upload moved host->device
    // 2-bit mode: bytes other than upper-case A/C/G/T are stored as code 0 plus an exception record
    // (position, byte), sorted by read then position; exc_off has one entry per read + 1
    std::vector<uint32_t> exc_off{0};
    std::vector<uint32_t> exc_pos;
    std::vector<uint8_t> exc_byte;
    std::vector<uint8_t> pair_state;  // per read pair: 0 = check codes on device, 1 = verified on host, 2 = not a pair
    uint64_t total_bases = 0;
    bool dirty = true;

    // device read set + tiling (built at upload)
    DevBuf d_words, d_woff, d_len, d_tiles, d_read_tile0, d_exc_off, d_exc_pos, d_exc_byte, d_pair_state;
    std::vector<uint32_t> h_read_tile0;  // n_reads + 1
    uint32_t n_tiles = 0;
    uint32_t max_len = 0;
    size_t n_exc_uploaded = 0;
    bool paired = false;  // every read 2i+1 is the reverse complement of read 2i (checked on device at upload)

    // per-call workspace (grow-only)
    DevBuf d_table, d_slot_cnt, d_slot_cur, d_slot_start, d_read_slot, d_chain, d_chain_tmp, d_long_list;
    DevBuf d_entry_off;   // wide index: offset o of every (read, phase) entry inside its read (k_wide_insert -> k_wide_chain_fill)
    DevBuf d_bloom, d_selfrep, d_tile_count, d_tile_off, d_truemask, d_ps_blocks, d_scalars, d_left, d_left_cnt, d_tile_extra;
    DevBuf d_cand_a, d_cand_p, d_cand_b, d_type, d_rowcnt, d_row_off, d_flag, d_pair_key, d_pair_min;
    DevBuf d_vlabel, d_vrank, d_vperm;  // verify order (k_read_label, k_read_sort, k_read_invert)
    DevBuf d_chain_state;               // ticket / done / status words of the single-pass scans (all-zero between launches)
    DevBuf d_tail_state;                // k_tile_rows / k_tail: row sums per tile of candidates + the done counter
    DevBuf spare_rows;   // device buffers of freed results, kept for the next call (hipFree / hipMalloc of a
    DevBuf spare_cands;  // 50-170 MB buffer costs ~0.2 ms each and synchronises the device)
    DevBuf spare_edges;
    DevBuf spare_nrank;   // the node-order buffer of the last edge result that was freed (po_result::d_nrank)
    DevBuf spare_spell;   // the byte buffer of the last po_spell result that was freed
    HostBuf spare_host;    // pinned row buffer of a freed result, kept for the next po_result_rows
    HostBuf scratch_host;  // pinned landing zone for small device->host copies into caller memory
    // pinned result pool sized while the reads are added (result_pool_grow): bytes of total_bases it was sized for
    uint64_t pool_bases = 0;
    // small device workspaces (<= 8 MB each, some forty of them) are carved out of 64 MB chunks instead of being
    // allocated one by one: on a process whose allocator has handed memory back, every small hipMalloc is a trip to
    // the kernel driver (0.2 ms each, 4 ms per first call of a handle)
    std::vector<void*> arena_chunks;
    char* arena_cur = nullptr;
    size_t arena_left = 0;
    int poison = -1;       // PHASM_POISON=<byte>: per-call workspaces are filled with it before every call
    // po_overlaps_to_host: a second stream copies chunk k's rows to the host while chunk k + 1 is computed
    hipStream_t copy_stream = nullptr;
    DevBuf chunk_rows[PO_MAX_PIECES + 1];
    // rows home in compact form (namespace home): chunk_compact[k] = chunk_rows[k] holds 16-byte records, not rows; the
    // records land in home_stage (page-locked; a bump allocator that starts over whenever the helper threads have caught up)
    bool chunk_compact[PO_MAX_PIECES + 1] = {};
    bool home_on = false;          // this po_overlaps_to_host call hands its rows home as records where the fused tail runs
    HostBuf home_stage;
    size_t home_used = 0;
    uint64_t home_seq = 0;         // pieces submitted to the helper threads by this call
    uint32_t home_gen = 0;         // number written behind a piece's copy (never repeats on a handle's landing zone)
    // records of 8 bytes instead of 16 where the read set allows it (po::pack_record): the shifts of this call (0 = 16-byte
    // records), and the state of the read set they were worked out for
    uint32_t home_sh_b = 0, home_sh_p = 0;
    uint64_t home_pack_n = ~0ull, home_pack_bases = ~0ull;
    uint32_t home_pack_b = 0, home_pack_p = 0;
    uint64_t home_last_bytes = 0;  // record bytes of the previous call (sizes home_stage)

    // streamed step (po_overlaps_to_host on a changed read set): the packed reads cross PCIe piece by piece on
    // up_stream while the pieces that have arrived go through the kernels and their rows travel back
    hipStream_t up_stream = nullptr;
    hipEvent_t ev_piece[PO_MAX_PIECES] = {};
    // the odd reads (reverse complements) of piece k are written on a stream of their own the moment the piece has landed,
    // beside whatever the handle's stream is doing for the piece before: ev_rc[k] = piece k is complete, both strands
    hipStream_t rc_stream = nullptr;
    hipEvent_t ev_rc[PO_MAX_PIECES] = {};
    hipEvent_t ev_meta = nullptr;
    hipEvent_t ev_first = nullptr;   // the first words of the later pieces are in place
    // first two packed words of every read, appended as the reads are added (registered memory: the streamed step sends
    // them ahead of the pieces straight from here); first_n = reads it covers (a bulk ingest fills it in afterwards)
    WordStore first_words;
    uint32_t first_n = 0;
    // ... and the first LEAD_WORDS words of every read, made when a streamed step first wants them (large read sets: the wide
    // index with windows of 4, whose K-mers reach into the fifth word); st_lead = words per read travelling ahead this step
    WordStore lead_words;
    uint32_t lead_n = 0;
    uint32_t st_lead = 2;
    // per-read metadata of the upload, kept page-locked while the read set is unchanged (reads are only ever appended):
    // [woff x n | len x n | first tile x (n + 1)]; meta_n = reads it covers, meta_bits = encoding it was counted for
    HostBuf meta_host;
    // Small host->device copies out of ordinary heap memory (a packed store below the registration size, the exception
    // records, the pair states) go through this page-locked block: handed a pageable source, the HIP runtime pins -- and
    // keeps a cache of the pin of -- whatever range of the PROCESS heap it lies in, next to the caller's own objects.
    HostBuf stage_host;
    size_t stage_used = 0;
    uint32_t meta_n = 0xFFFFFFFFu;
    int meta_bits = 0;
    uint64_t elig_n = ~0ull, elig_val = 0;   // reads of length >= elig_m among the first elig_n (cache of a 100 k-iteration loop)
    uint32_t elig_m = 0;
    DevBuf d_first, d_defer;
    uint32_t defer_need = 0;       // deferred containment candidates the last streamed call produced
    // a piece whose kernels are queued but whose row count has not been read yet (run_overlaps returned without the
    // closing synchronisation: the next piece's first host wait covers it, st_harvest then sends its rows home)
    struct Pending {
        bool valid = false;
        uint32_t k = 0;
        po_stats S = {};
        bool ver_timed = false;
        bool full_events = true;
        bool pair_events = true;
        bool tail = false;         // the piece's tail ran as k_tail: counts in pinned[zone..], fallback flag in pinned[zone + 7]
        bool compact = false;      // ... as k_tail_cands: the piece's buffer holds records
        int zone = 48;
        uint32_t cap_c = 0;        // > 0: the candidate count was predicted (real count in pinned[zone + 8])
        hipEvent_t* ev = nullptr;
    } st_pend;
    std::function<po_status()> st_harvest;
    // candidates per piece of the last streamed call, valid for the same reads, cuts and min_length (st_pred_sig)
    uint64_t st_pred_cand[PO_MAX_PIECES] = {};
    std::vector<uint32_t> st_pred_sig;
    bool st_pred_valid = false;
    bool st_selfclean = false;     // the previous piece of this streamed step left the per-call counters zero (no reset launch needed)
    bool st_early_index = false;   // this streamed step builds its index before piece 0 has landed
    bool st_tail_gave_up = false;  // the last streamed step was abandoned because of tandem-repeat reads (statistics / tests)
    uint32_t st_defer_cap = 0;
    uint64_t last_host_rows = 0;   // rows of the previous po_overlaps_to_host call (sizes the pinned buffer up front)
    // the anchor index of the last call, reusable while the device copy of the reads and the parameters it was built
    // for are unchanged (the chunks of po_overlaps_to_host, the shards of a multi-GPU step, repeated calls)
    uint64_t upload_gen = 0;
    bool idx_valid = false;
    uint64_t idx_gen = 0;
    uint32_t idx_m = 0, idx_tbits = 0, idx_bits = 0, idx_ww = 0;
    bool idx_wide = false;
    // sliced wide index (multi-GPU, phasm_amd/dist.py IndexExchange): what the last slice build (OverlapArgs::build_n > 1)
    // left in the workspaces for po_index_slice_export
    bool sl_is_wide = false;
    uint32_t sl_tbits = 0;
    uint64_t sl_entries = 0;
    // sharded upload (multi-GPU): store 0 arrives as nshards pieces that other ranks uploaded and xGMI carried here
    const uint64_t* asm_pieces = nullptr;
    uint64_t asm_slot_words = 0;
    uint32_t asm_n = 0, asm_parts = 1;
    DevBuf d_end_a, d_end_b, d_dpcnt;
    int live_results = 0;

    po_stats stats = {};

    // layout stage 1 (po_layout_edges)
    bool segments_only = false;  // reads were added by po_add_segment: lengths and names, no sequence
    int ids_paired = -1;         // -1 unknown, 0/1: ids come in (name+"+", name+"-") pairs
    hipEvent_t ev_lay[EV_LAY_N] = {};  // one slice per layout call: EV_EDGES, EV_REDUCE, ... (the enum beside EV_LAY_N)
    DevBuf d_lay_len, d_lay_cnt, d_rflag, d_removed, d_ekey, d_ecnt, d_ewin, d_eoff;
    DevBuf d_efirst;             // table path: first writer row per winning row (the edges' rank, po_result::d_rank)
    po_layout_stats lstats = {};

    // transitive reduction + symmetry pass (po_layout_reduce, reduce.hip.h)
    DevBuf d_red[RB_N];
    po_reduce_stats rstats = {};

    // the node order of the stage-1 graph (k_layout_node_rank) and tip removal (po_layout_tips, tips.hip.h)
    DevBuf d_lay_firstc;
    DevBuf d_tip[TB_N];
    po_tips_stats tstats = {};
    po_diamond_stats dstats = {};   // po_layout_diamonds (diamond.hip.h) works in the buffers of d_tip: one call at a time
    po_node_order_stats nostats = {};

    // merging of unambiguous paths (po_layout_merge, merge.hip.h)
    DevBuf d_mrg[MB_N];
    po_merge_stats mstats = {};

    // average coverage per edge (po_layout_coverage, coverage.hip.h)
    DevBuf d_cov[VB_N];
    po_coverage_stats cstats = {};

    // the ranks of a graph result, recomputed by every call of the two stages below (ranked_open)
    DevBuf d_rank[RK_N];
    // weakly connected components (po_layout_components, components.hip.h)
    DevBuf d_cc[KB_N];
    po_components_stats ccstats = {};
    // strongly connected components and the superbubble partition (po_layout_partition, partition.hip.h)
    DevBuf d_scc[PB_N];
    po_partition_stats pstats = {};
    // the superbubbles of the acyclic partitions (po_layout_superbubbles, superbubbles.hip.h)
    DevBuf d_sb[UB_N];
    po_superbubble_stats sbstats = {};
    // the superbubbles of the whole graph, the cyclic partitions included (po_layout_superbubbles_all, cyclic.hip.h)
    DevBuf d_cy[YB_N];
    po_superbubble_all_stats sastats = {};
    // the bubble chains (po_layout_bubblechains, bubblechains.hip.h)
    DevBuf d_bc[HB_N];
    po_bubblechain_stats bcstats = {};
    po_bubblechain_all_stats bcastats = {};   // (po_layout_bubblechains_all: the same stage behind po_layout_superbubbles_all's)
    // the contigs outside the bubble chains (po_layout_contigs, contigs.hip.h)
    DevBuf d_ct[CB_N];
    po_contig_stats ctstats = {};
    // scoring and pruning of the haplotype extensions at one bubble (po_phase_branch, phase.hip.h)
    DevBuf d_ph[FB_N];
    po_phase_stats phstats = {};
    // where the last run_phase left its final list and the paths' bitsets (in d_ph, until the next call that works there):
    // what po_walk_step takes over
    const uint32_t *ph_fcand = nullptr, *ph_fext = nullptr, *ph_pbits = nullptr;
    const double* ph_frl = nullptr;
    po_walk_stats wkstats = {};
    // the alignment index and the relevant reads of a bubble (po_phase_index, po_phase_relevant, relevant.hip.h)
    DevBuf d_rr[XB_N];
    po_phase_index_stats pxstats = {};
    po_relevant_stats rvstats = {};
    // the sequences of graph paths out of the resident reads (po_spell, spell.hip.h)
    DevBuf d_sp[SB_N];
    po_spell_stats spstats = {};
    // paths, interior and exit predecessors of every top-level bubble (po_phase_paths, paths.hip.h)
    DevBuf d_pp[QB_N];
    po_paths_stats ppstats = {};
    // every listed path of a large bubble scored, the best of them named (po_phase_large, large.hip.h)
    DevBuf d_lg[LB_N];
    po_large_stats lgstats = {};
};

struct po_result {
    po_handle* h = nullptr;
    DevBuf d_rows;          // po_row[count] (elem 24) or po_cand[count] (elem 16)
    uint64_t count = 0;
    size_t elem = sizeof(po_row);
    bool kind_edges = false;  // po_edge entries (same size as po_cand)
    void* host = nullptr;     // host copy of the entries: pinned (hipHostMalloc, host_cap bytes) unless host_malloced
    size_t host_cap = 0;
    bool host_malloced = false;  // po_result_from_rows: plain malloc (works without a GPU)
    // rows written by this library's paired-strand emission: every (row, strand mirror) group is the only writer of
    // its twin edge pair -- po_layout_edges needs no dedupe table for them (layout.hip.h, k_layout_winner_adjacent)
    bool unique_twins = false;
    // po_layout_edges through the table: the first writer row of every edge, its place in the reference's adjacency
    // OrderedDict (po_layout_reduce orders by it; empty = the emission order is that order already)
    DevBuf d_rank;
    // edge results: (first reaching row << 2 | slot) per node, the place of the node in the reference's graph order
    // (layout.hip.h, k_layout_node_rank; all ones = the node is not in the graph); po_layout_tips walks in this order
    DevBuf d_nrank;
    // po_layout_merge: a merged graph -- node ids >= the handle's reads name merged nodes (d_nrank holds their ranks too);
    // the tables of po_result_merged_paths
    bool merged = false;
    // po_graph_from_edges: edges and node order came from the caller, not from the rows (po_layout_components takes it;
    // the stages that clean, merge or cover a graph do not)
    bool host_graph = false;
    uint64_t n_merged = 0, n_members = 0;
    DevBuf d_moff, d_member, d_prefix, d_mlen;
    // po_candidates_shard_into: the caller's buffer the candidates go to when they fit
    void* ext_dst = nullptr;
    uint64_t ext_cap = 0;
    bool wrote_ext = false;
    // po_phase_index (special == 1) and po_phase_relevant (special == 2): results of a kind of their own -- elem is 1 and
    // count 0, so every call that wants rows, candidates or edges refuses them by its own check.
    // The index: key table, value words (the place of the key's entry), offsets per read, entries, read lengths.
    uint8_t special = 0;
    uint32_t ix_n_ids = 0, ix_n_slots = 0, ix_n_keys = 0;
    DevBuf d_ixtable, d_ixval, d_ixoff, d_ixent, d_ixlen;
    // The relevant reads of one bubble, on the host (they are bubble-sized)
    po_relevant_dims rv = {};
    std::vector<uint32_t> rv_ca, rv_rel, rv_alnoff, rv_alnb, rv_b;
    std::vector<int32_t> rv_om, rv_a0, rv_a1;
    // po_spell (special == 3): d_rows holds the bytes of all sequences back to back (padded to whole 16-byte chunks), sp_off
    // the n_seqs + 1 byte offsets of the sequences
    std::vector<uint64_t> sp_off;
    // po_phase_paths (special == 4): everything stays in HBM (d_pp, 32-bit offsets: the call refuses what does not fit them)
    DevBuf d_pp[PR_N];
    po_paths_dims pp = {};
    // the node ids of its graph are below pp_n_total; the table, inside_off and bubble_path_off on the host once
    // po_phase_large or po_paths_copy_paths asked for them (they are bubble-sized)
    uint32_t pp_n_total = 0;
    std::vector<po_bubble_paths> pp_table;
    std::vector<uint32_t> pp_inoff, pp_bpo;
    // po_walk_create (special == 5): the candidate sets of a walk along a bubble chain (walk.hip.h).  On the device: the bit
    // rows of the slots over block-stable read ids and the log_rl of the candidates, each as a ping-pong pair (wk_cur names
    // the live half), and the links (parent, extension) of every advanced bubble, level after level (wk_level_off).  On the
    // host: the block reads in the order they joined (stable id -> global id) and the same sorted by global id.
    uint32_t wk_k = 0, wk_n_cands = 1, wk_W = 0;
    int wk_cur = 0;
    DevBuf d_wk_rows[2], d_wk_rl[2], d_wk_links, d_wk_tmp;
    std::vector<uint64_t> wk_level_off;                          // depth + 1 entries once a bubble was advanced
    std::vector<uint32_t> wk_reads;                              // stable id -> global id
    std::vector<std::pair<uint32_t, uint32_t>> wk_sorted;        // (global id, stable id), ascending
    // The RESIDENT route of a walk (po_walk_relevant, po_walk_step_resident; resident.hip.h).  wk_route: which route the block
    // advanced by (0 none yet, 1 the host map wk_sorted, 2 the device map).  On the device: the workspaces and outputs of the
    // walk's one live gather (d_rs_rel, the XB_* of po_phase_relevant), the bitsets prev_graph and prev_aligning over the
    // handle's read ids, stable_of[global id] and global_of[stable id], and the step's scratch (flags, ranks, translation,
    // the rewritten aln_b, the path ids).  rs_n_block: the block reads of route 2.  A reset only notes what the next device
    // call has to clear: rs_unmap_n entries of global_of to un-map, rs_clear_prev the two bitsets.
    uint8_t wk_route = 0;
    DevBuf d_rs_rel[XB_N], d_rs_prev, d_rs_stable, d_rs_global, d_rs_step[6];
    uint32_t rs_n_ids = 0, rs_n_block = 0, rs_unmap_n = 0, rs_prevg_bound = 0;
    bool rs_clear_prev = false;
    po_result* rs_live = nullptr;                                // the gather result that names d_rs_rel, if one does
    // A gather result of po_walk_relevant (special == 2 with rv_walk set): the arrays stay in the walk's d_rs_rel.
    po_result* rv_walk = nullptr;                                // the walk it belongs to (nulled when that walk is freed)
    bool rv_resident = false, rv_stale = false, rv_empty = false, rv_used_prev = false;
    uint32_t rv_depth = 0, rv_resets = 0, rv_mode = 0;
    bool compact = false;   // (inside po_overlaps_to_host only) d_rows holds the verified-candidate records of `count` ROWS
};

namespace {

po_status fail(po_handle* h, po_status st, const std::string& msg) {
    if (h) h->err = msg;
    return st;
}

#define HIP_TRY(h, expr)                                                                        \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) {                                                                 \
            return fail((h), e_ == hipErrorOutOfMemory ? PO_ERR_NOMEM : PO_ERR_HIP,             \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                     \
        }                                                                                       \
    } while (0)

// PHASM_ALLOC_TRACE=1: every allocation / registration a call makes, with its wall time, on stderr (developer aid:
// what a COLD call -- the first one on a handle -- pays that the steady state does not)
struct AllocTrace {
    const char* what;
    size_t bytes;
    std::chrono::steady_clock::time_point t0;
    bool on;
    AllocTrace(const char* w, size_t b) : what(w), bytes(b), on(getenv("PHASM_ALLOC_TRACE") != nullptr) {
        if (on) t0 = std::chrono::steady_clock::now();
    }
    ~AllocTrace() {
        if (on)
            std::fprintf(stderr, "[alloc] %-16s %10.3f MB  %8.3f ms\n", what, bytes / 1e6,
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
};

// What a caller wants from run_overlaps.  Every call mode travels here and nowhere else: run_overlaps can see what it was
// called with, and nothing a call was asked for is left on the handle for the next one.
struct OverlapArgs {
    uint32_t min_length = 0, shard = 0, nshards = 1;
    bool want_cands = false;   // the multi-GPU form: verified candidates (one per strand-mirror pair) instead of rows
    // a piece of a streamed step: reads [r_begin, r_end), `shard` is the piece's number.  idx_only: stop behind the index
    // build (the step builds it ahead of piece 0).  ws_scale > 1: per-piece workspaces are sized for the step's LARGEST
    // piece when the first one asks, so that no later piece has to free and re-allocate (hipFree synchronises the device)
    bool streamed = false, idx_only = false;
    uint32_t r_begin = 0, r_end = 0;
    double ws_scale = 1.0;
    // sliced wide index (multi-GPU, phasm_amd/dist.py IndexExchange): build_n > 1 builds sub-table build_slice and stops;
    // ext_index probes a gathered sliced index (its geometry in the four words behind it) instead of building one
    uint32_t build_slice = 0, build_n = 0;
    const void* ext_index = nullptr;
    uint32_t ext_slices = 0, ext_tbits = 0, ext_chunk_slots = 0, ext_chain_off = 0;
    // po_overlaps_ex: the verify step is the banded DP of extend.hip.h, at most dp_E differences in a band of dp_W
    bool dp = false;
    uint32_t dp_E = 0, dp_W = 0;
};

po_status ensure(po_handle* h, DevBuf& b, size_t bytes, double scale = 1.0, bool arena_ok = true, bool streamed = false) {
    if (bytes <= b.cap) return PO_OK;
    AllocTrace tr("hipMalloc", bytes);
    const bool first = b.p == nullptr;
    b.release();
    size_t want = bytes + bytes / 8 + 256;
    if (scale > 1.0) want = (size_t)((double)bytes * scale) + 256;   // (a streamed piece: room for the largest piece)
    if (streamed) want += 8192;   // (... and for the next call's predicted count plus its slack, small inputs included)
    constexpr size_t ARENA_CHUNK = 64u << 20, ARENA_MAX = 8u << 20;
    // (arena_ok = false: buffers that leave the handle with a result -- rows, candidates, edges -- are freed or kept as
    // spares one by one; carved out of a chunk they would stay behind until the handle dies)
    if (h && first && arena_ok && want <= ARENA_MAX && !getenv("PHASM_NO_ARENA")) {
        // (only a buffer's FIRST allocation: one that has to grow moves out, so a chunk never fills up with dead pieces)
        want = (want + 255) & ~size_t(255);
        if (h->arena_left < want) {
            void* c = nullptr;
            if (hipMalloc(&c, ARENA_CHUNK) == hipSuccess) {
                h->arena_chunks.push_back(c);
                h->arena_cur = static_cast<char*>(c);
                h->arena_left = ARENA_CHUNK;
            } else {
                (void)hipGetLastError();
            }
        }
        if (h->arena_left >= want) {
            b.p = h->arena_cur;
            b.cap = want;
            b.arena = true;
            h->arena_cur += want;
            h->arena_left -= want;
            if (h->poison >= 0 && h->stream) (void)hipMemsetAsync(b.p, h->poison, want, h->stream);
            return PO_OK;
        }
    }
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) {
        b.p = nullptr;
        return fail(h, PO_ERR_NOMEM, "hipMalloc(" + std::to_string(want) + " bytes): " + hipGetErrorString(e));
    }
    b.cap = want;
    // PHASM_POISON: a fresh allocation starts out as garbage of the caller's choosing (hipMalloc usually hands out
    // zeros or whatever an earlier handle of the process left there): a kernel that reads what this call has not
    // written shows up as a parity failure instead of depending on the history of the process
    if (h && h->poison >= 0 && h->stream) (void)hipMemsetAsync(b.p, h->poison, want, h->stream);
    return PO_OK;
}

// a workspace whose size follows the candidate count of the a-side range at hand
po_status ensure_piece(po_handle* h, DevBuf& b, size_t bytes, const OverlapArgs& a) { return ensure(h, b, bytes, a.ws_scale, true, a.streamed); }

po_status ensure_host(po_handle* h, HostBuf& b, size_t bytes) {
    if (bytes <= b.cap) return PO_OK;
    AllocTrace tr("hipHostMalloc", bytes);
    b.release();
    const size_t want = bytes + bytes / 16 + 4096;
    hipError_t e = hipHostMalloc(&b.p, want, hipHostMallocDefault);
    if (e != hipSuccess) {
        b.p = nullptr;
        return fail(h, PO_ERR_NOMEM, "hipHostMalloc(" + std::to_string(want) + " bytes): " + hipGetErrorString(e));
    }
    b.cap = want;
    pin_note(b.p, want, 1u);
    return PO_OK;
}

// the packed host store is about to change (it may move, and the old block is unregistered and freed): no copy out of
// it may be in flight
void quiesce_store(po_handle* h) {
    if (!h->dev_ready) return;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    if (h->up_stream) (void)hipStreamSynchronize(h->up_stream);
    if (h->rc_stream) (void)hipStreamSynchronize(h->rc_stream);
}

// Pinned result pool, sized WHILE THE READS ARE ADDED.  A fresh 170 MB page-locked array costs 8 ms (hipHostMalloc maps
// and pins every page), more than the whole steady-state call: a cold call that allocates it -- let alone grows it
// twice, as the first call on a handle used to -- pays several times the step.  How many rows a call will return is
// not known before the scan, so the pool is a guess made from what IS known, the bases added so far: one row per
// 160 oriented bases (BASELINE config 2 gives one per 214, config 3 one per 320, config 5 one per 436), re-made
// whenever the read set has grown by half, capped at 4 GB.  A call that needs more grows the array as before.
po_status init_device(po_handle* h);

inline bool home_enabled() {
    const char* e = getenv("PHASM_HOME");
    return !(e && atoi(e) == 0);
}

void result_pool_grow(po_handle* h, uint64_t bases = 0) {
    if (!bases) bases = h->total_bases;   // (bases > 0: an estimate made before the reads are in -- po_add_fasta's warm-up thread)
    h->pool_bases = bases + bases / 2;   // next look when the set has grown by half
    if (getenv("PHASM_NO_POOL")) return;
    // a read set this size is headed for the GPU: bring the device up now (runtime start, stream, events: 130 ms in a
    // fresh process) rather than inside the first call.  No GPU: the call itself will say so.
    if (!h->dev_ready && init_device(h) != PO_OK) h->err.clear();
    const uint64_t want = std::min<uint64_t>(h->pool_bases / 160 * sizeof(po_row), 4ull << 30);
    if (h->spare_host.cap >= want || h->live_results) return;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
        (void)hipGetLastError();
        h->pool_bases = ~0ull;   // no GPU here: never ask again
        return;
    }
    AllocTrace tr("result pool", want);
    h->spare_host.release();
    if (hipHostMalloc(&h->spare_host.p, want, hipHostMallocPortable) == hipSuccess) {
        h->spare_host.cap = want;
        pin_note(h->spare_host.p, want, 1u);
        // the landing block of the compact records (a third of the row bytes), sized with it -- not inside the first call
        if (home_enabled() && h->home_stage.cap < want / 3) (void)ensure_host(h, h->home_stage, want / 3);
        // and the first LARGE copy in each direction (the copy engines' queues are made by it: the first piece of the first
        // call of a process took 7.5 ms instead of 0.5) moves 8 MB of the fresh pool to the device and back
        if (h->dev_ready && h->up_stream && h->copy_stream && want >= (16u << 20) && !getenv("PHASM_NO_WARM")) {
            void* w = nullptr;
            const size_t nb = 8u << 20;
            if (hipMalloc(&w, nb) == hipSuccess) {
                (void)hipMemcpyAsync(w, h->spare_host.p, nb, hipMemcpyHostToDevice, h->up_stream);
                (void)hipStreamSynchronize(h->up_stream);
                (void)hipMemcpyAsync(static_cast<char*>(h->spare_host.p) + nb, w, nb, hipMemcpyDeviceToHost, h->copy_stream);
                (void)hipStreamSynchronize(h->copy_stream);
                (void)hipFree(w);
            }
            (void)hipGetLastError();
        }
    } else {
        (void)hipGetLastError();
        h->spare_host.p = nullptr;
        h->pool_bases = ~0ull;
    }
}

#define PO_TRY(expr)                    \
    do {                                \
        po_status s_ = (expr);          \
        if (s_ != PO_OK) return s_;     \
    } while (0)

// Streams, events and the small page-locked landing zone of a handle are kept for the NEXT handle of the process instead
// of being destroyed with this one: a test process (and a server) creates and destroys handles by the hundred, each with
// four streams and ~70 events -- churn inside the HIP runtime (its completion handlers run on threads of their own) that
// buys nothing, and ~1 ms of a fresh handle's first call.  A kit is idle when it is put back (every stream synchronised).
struct DevKit {
    int device = -1;
    hipStream_t stream = nullptr, copy_stream = nullptr, up_stream = nullptr, rc_stream = nullptr;
    hipEvent_t ev_sets[2][EV_N] = {};
    hipEvent_t ev_up0 = nullptr, ev_up1 = nullptr, ev_meta = nullptr, ev_first = nullptr;
    hipEvent_t ev_piece[PO_MAX_PIECES] = {}, ev_rc[PO_MAX_PIECES] = {}, ev_lay[EV_LAY_N] = {};

    uint64_t* pinned = nullptr;
    uint64_t* pinned_dev = nullptr;
};
static_assert(sizeof(DevKit::ev_lay) == sizeof(po_handle::ev_lay), "a kit carries every layout event of a handle");
std::mutex g_kit_mu;
std::vector<DevKit> g_kits;
constexpr size_t KIT_POOL_MAX = 8;

bool kit_take(po_handle* h) {
    std::lock_guard<std::mutex> lock(g_kit_mu);
    for (size_t i = 0; i < g_kits.size(); ++i) {
        if (g_kits[i].device != h->device) continue;
        const DevKit k = g_kits[i];
        g_kits.erase(g_kits.begin() + (long)i);
        h->stream = k.stream;
        h->copy_stream = k.copy_stream;
        h->up_stream = k.up_stream;
        h->rc_stream = k.rc_stream;
        std::memcpy(h->ev_sets, k.ev_sets, sizeof(k.ev_sets));
        h->ev_up0 = k.ev_up0;
        h->ev_up1 = k.ev_up1;
        h->ev_meta = k.ev_meta;
        h->ev_first = k.ev_first;
        std::memcpy(h->ev_piece, k.ev_piece, sizeof(k.ev_piece));
        std::memcpy(h->ev_rc, k.ev_rc, sizeof(k.ev_rc));
        std::memcpy(h->ev_lay, k.ev_lay, sizeof(k.ev_lay));
        h->pinned = k.pinned;
        h->pinned_dev = k.pinned_dev;
        return true;
    }
    return false;
}

// true: the handle's streams / events / landing zone went back to the pool (the caller must not destroy them)
bool kit_give(po_handle* h) {
    if (getenv("PHASM_NO_KIT_POOL") || !h->stream || !h->copy_stream || !h->up_stream || !h->rc_stream || !h->pinned) return false;
    if (hipStreamSynchronize(h->stream) != hipSuccess || hipStreamSynchronize(h->copy_stream) != hipSuccess ||
        hipStreamSynchronize(h->up_stream) != hipSuccess || hipStreamSynchronize(h->rc_stream) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    DevKit k;
    k.device = h->device;
    k.stream = h->stream;
    k.copy_stream = h->copy_stream;
    k.up_stream = h->up_stream;
    k.rc_stream = h->rc_stream;
    std::memcpy(k.ev_sets, h->ev_sets, sizeof(k.ev_sets));
    k.ev_up0 = h->ev_up0;
    k.ev_up1 = h->ev_up1;
    k.ev_meta = h->ev_meta;
    k.ev_first = h->ev_first;
    std::memcpy(k.ev_piece, h->ev_piece, sizeof(k.ev_piece));
    std::memcpy(k.ev_rc, h->ev_rc, sizeof(k.ev_rc));
    std::memcpy(k.ev_lay, h->ev_lay, sizeof(k.ev_lay));
    k.pinned = h->pinned;
    k.pinned_dev = h->pinned_dev;
    std::lock_guard<std::mutex> lock(g_kit_mu);
    if (g_kits.size() >= KIT_POOL_MAX) return false;
    g_kits.push_back(k);
    return true;
}


// CPUs this process may use: the hardware's count, cut to the container's CPU quota where there is one (cgroup v2 cpu.max
// "quota period", v1 cpu.cfs_quota_us / _period_us) -- hardware_concurrency() says 256 on a box whose process may use 16, and
// threads beyond the share only get the whole process throttled
unsigned cpu_share() {
    static const unsigned share = [] {
        unsigned n = std::thread::hardware_concurrency();
        n = n ? n : 4u;
        long long q = -1, per = 100000;
        if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
            char buf[64] = {0};
            if (std::fscanf(f, "%63s %lld", buf, &per) >= 1 && std::strcmp(buf, "max") != 0) q = atoll(buf);
            std::fclose(f);
        } else if (FILE* g = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {
            if (std::fscanf(g, "%lld", &q) != 1) q = -1;
            std::fclose(g);
            if (FILE* g2 = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
                if (std::fscanf(g2, "%lld", &per) != 1) per = 100000;
                std::fclose(g2);
            }
        }
        if (q > 0 && per > 0) n = std::min<unsigned>(n, (unsigned)std::max<long long>(1, q / per));
        return n;
    }();
    return share;
}

// ---- rows home in compact form -------------------------------------------------------------------------------------------
// po_overlaps_to_host used to bring every 24-byte row across PCIe: 168 MB at BASELINE config 2, and the step ended when that
// copy ended.  Half of those rows are strand mirrors of the other half, and every exact row is a function of {a, p, b, type}
// and the two read lengths -- the verified-candidate record the multi-GPU exchange already uses (po_cand, 16 bytes), or ONE
// 64-bit word where the read set allows it (po::pack_record: 23 MB at config 2).  So the device hands out one record per
// strand-mirror pair (k_tail_cands), the records cross PCIe, and host threads write the rows into the page-locked result
// array while later pieces are still on the device: the same array, byte for byte, that k_tail / k_emit write on the device
// (rows per record in write_rows' order: A row, [its mirror], B row, [its mirror]; records in candidate order).  SURVEY.md
// section 8c has the mirror rules; the row fields are those of src/overlapper.cpp:77-82,104-110.
//
// One pool per process, threads started at the first use (three quarters of the process's CPU share, 12 at most;
// PHASM_HOME_THREADS).  Helpers sleep between pieces and spin inside one (a piece is 50-400 us of work).  Thread 0 takes the
// pieces in order: it polls the page-locked word a one-thread kernel writes behind the piece's device->host copy, then all
// threads count the rows of the piece's chunks (CHUNK records each), thread 0 turns the counts into offsets -- and checks the
// total against what the device counted --, and all threads write.
namespace home {

constexpr uint32_t CHUNK = 4096;

struct Job {
    const void* rec = nullptr;       // page-locked staging memory: po::Cand records, or (sh_b != 0) packed 8-byte records
    uint32_t sh_b = 0, sh_p = 0;     // po::pack_record's shifts
    uint64_t n_rec = 0;
    po_row* out = nullptr;           // where this piece's rows start in the result array
    uint64_t n_rows = 0;             // what the device counted for the piece
    // the piece's records are home when *flag == want: a one-thread kernel queued behind their device->host copy on the
    // copy stream writes `want` into page-locked memory (polling a word costs the caller's launches nothing; polling
    // hipEventQuery takes the runtime's locks on every call).  flag == nullptr: the records are there already.
    const volatile uint32_t* flag = nullptr;
    uint32_t want = 0;
    // the read set's form: strand-mirror pairs (rows_of_rec), bits per base (the byte counters).  Per job, so that the
    // caller never writes state the threads may still be reading for the piece before
    uint32_t paired = 0, bits = 2;
};

struct Pool {
    std::vector<std::thread> thr;
    std::mutex mu;                   // queue, job hand-over, sleep / wake
    std::condition_variable cv_queue;   // thread 0: a piece was submitted
    std::condition_variable cv_job;     // helpers: a piece was published
    std::mutex call_mu;              // one call at a time uses the pool
    std::deque<Job> queue;
    std::atomic<uint64_t> submitted{0}, finished{0};
    std::atomic<int> error{0};       // 1: counts disagree, 2: a record names an unknown read
    // the call's read set
    const uint32_t* len = nullptr;
    uint32_t n_reads = 0;
    // byte counters of po_stats over the call's records (k_emit / k_tail sum them on the device for rows emitted there)
    std::atomic<uint64_t> sum_l{0}, sum_b{0}, sum_e{0};
    // the piece being expanded
    Job cur;
    uint64_t job_seq = 0;            // (under mu) pieces published so far
    uint32_t n_chunks = 0;
    std::vector<uint64_t> chunk_off;
    std::atomic<uint32_t> next_count{0}, done_count{0}, next_write{0}, done_write{0};
    std::atomic<int> phase{0};       // 0: none, 1: count, 2: write
    std::atomic<int> inside{0};      // helper threads inside the current piece's loops
    // PHASM_STREAM_TRACE: per piece, microseconds since the call began -- records home / rows written
    std::chrono::steady_clock::time_point t0;
    std::vector<std::array<double, 3>> trace;   // {ready, done, rows}
    bool tracing = false;
};

Pool* g_pool = nullptr;
std::once_flag g_pool_once;

inline void cpu_pause() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#endif
}

// Spin until pred() holds.  The waits of a piece are microseconds long when every thread has a core; on a host whose cores
// are busy with other people's work a thread can spin through the time slice of the very thread it waits for (a box like
// that gave 5.2-5.5 ms per step instead of 4.7), so after a few thousand pauses the waiter offers its core.
std::atomic<uint32_t> g_spin_limit{4096};   // pauses before a waiter starts yielding (PHASM_HOME_SPIN; 0 = never yield)
template <class Pred>
inline void spin_until(Pred pred) {
    const uint32_t limit = g_spin_limit.load(std::memory_order_relaxed);
    for (uint32_t n = 0; !pred(); ++n) {
        if (limit == 0 || n < limit) cpu_pause();
        else std::this_thread::yield();
    }
}

inline po::Cand load_rec(const Job& j, uint64_t i) {
    if (!j.sh_b) return static_cast<const po::Cand*>(j.rec)[i];
    return po::unpack_record(static_cast<const uint64_t*>(j.rec)[i], j.sh_b, j.sh_p);
}

inline uint32_t rows_of_rec(const po::Cand& c, uint32_t paired) {
    if (!paired) return (c.type & 1u) + ((c.type >> 1) & 1u);
    return ((c.type & 1u) ? (c.a == (c.b ^ 1u) ? 1u : 2u) : 0u) + ((c.type & 2u) ? 2u : 0u);
}

inline void put_row(uint64_t*& o, uint32_t a, uint32_t b, uint32_t astart, uint32_t aend, uint32_t bend) {
    // (a row is three 8-byte words; non-temporal stores: the array is written once and read by the caller much later)
    __builtin_nontemporal_store((uint64_t)a | ((uint64_t)b << 32), o);
    __builtin_nontemporal_store((uint64_t)astart | ((uint64_t)aend << 32), o + 1);
    __builtin_nontemporal_store((uint64_t)bend << 32, o + 2);
    o += 3;
}

// rows of records [lo, hi) -> out; returns false when a record names a read the handle does not hold
// (the byte counters of po_stats -- write_rows' counters, kernels.hip.h -- are taken here, where the two lengths are at hand:
// the counting pass in front of this one then needs nothing but the records)
bool expand_records(Pool& P, uint64_t lo, uint64_t hi, po_row* out) {
    uint64_t* o = reinterpret_cast<uint64_t*>(out);
    const Job& job = P.cur;
    const uint32_t* len = P.len;
    const uint32_t paired = job.paired, n_reads = P.n_reads, bits = job.bits;
    auto pb = [bits](uint32_t l) -> uint64_t { return bits == 8u ? l : (l >> 2) + ((l & 3u) != 0u); };
    uint64_t sl = 0, sb = 0, se = 0;
    for (uint64_t i = lo; i < hi; ++i) {
        const po::Cand c = load_rec(job, i);
        if (c.a >= n_reads || c.b >= n_reads) return false;
        const uint32_t la = len[c.a], lb = len[c.b];
        se += 2 * pb((c.type & 1u) ? la - c.p : lb);
        if (c.type & 1u) {
            const uint32_t l = la - c.p;
            const bool twin = paired && c.a != (c.b ^ 1u);
            put_row(o, c.a, c.b, c.p, la, l);
            if (twin) put_row(o, c.b ^ 1u, c.a ^ 1u, lb - l, lb, l);
            const uint64_t k = twin ? 2 : 1;
            sl += k * l;
            sb += k * 2 * pb(l);
        }
        if (c.type & 2u) {
            put_row(o, c.a, c.b, c.p, c.p + lb, lb);
            if (paired) put_row(o, c.a ^ 1u, c.b ^ 1u, la - c.p - lb, la - c.p, lb);
            const uint64_t k = paired ? 2 : 1;
            sl += k * lb;
            sb += k * 2 * pb(lb);
        }
    }
    P.sum_l.fetch_add(sl, std::memory_order_relaxed);
    P.sum_b.fetch_add(sb, std::memory_order_relaxed);
    P.sum_e.fetch_add(se, std::memory_order_relaxed);
    return true;
}

// the two passes over the current piece; `lead` (thread 0) turns the counts into offsets between them.  A piece is
// 50-400 us of work for the pool: inside it the threads spin, between pieces they sleep.
void run_phases(Pool& P, bool lead) {
    const uint32_t nc = P.n_chunks;
    for (;;) {   // count
        const uint32_t c = P.next_count.fetch_add(1, std::memory_order_relaxed);
        if (c >= nc) break;
        const uint64_t lo = (uint64_t)c * CHUNK, hi = std::min<uint64_t>(P.cur.n_rec, lo + CHUNK);
        uint64_t n = 0;
        const uint32_t paired = P.cur.paired;
        for (uint64_t i = lo; i < hi; ++i) n += rows_of_rec(load_rec(P.cur, i), paired);
        P.chunk_off[c + 1] = n;
        P.done_count.fetch_add(1, std::memory_order_release);
    }
    if (lead) {
        spin_until([&] { return P.done_count.load(std::memory_order_acquire) >= nc; });
        P.chunk_off[0] = 0;
        for (uint32_t c = 0; c < nc; ++c) P.chunk_off[c + 1] += P.chunk_off[c];
        if (P.chunk_off[nc] != P.cur.n_rows) P.error.store(1);   // (the device counted differently: nothing is written)
        P.phase.store(P.error.load() ? 0 : 2, std::memory_order_release);
    } else {
        spin_until([&] { return P.phase.load(std::memory_order_acquire) != 1; });
    }
    if (P.phase.load(std::memory_order_acquire) != 2) return;
    for (;;) {   // write
        const uint32_t c = P.next_write.fetch_add(1, std::memory_order_relaxed);
        if (c >= nc) break;
        const uint64_t lo = (uint64_t)c * CHUNK, hi = std::min<uint64_t>(P.cur.n_rec, lo + CHUNK);
        if (!expand_records(P, lo, hi, P.cur.out + P.chunk_off[c])) P.error.store(2);
#if defined(__x86_64__)
        __builtin_ia32_sfence();   // (non-temporal stores are ordered by sfence only: before the chunk counts as written)
#endif
        P.done_write.fetch_add(1, std::memory_order_release);
    }
}

void helper(Pool* Pp) {
    Pool& P = *Pp;
    uint64_t seen = 0;
    for (;;) {
        {
            std::unique_lock<std::mutex> lock(P.mu);
            P.cv_job.wait(lock, [&] { return P.job_seq != seen; });
            seen = P.job_seq;
        }
        P.inside.fetch_add(1, std::memory_order_acq_rel);
        if (P.phase.load(std::memory_order_acquire) != 0) run_phases(P, false);
        P.inside.fetch_sub(1, std::memory_order_release);
    }
}

void leader(Pool* Pp) {
    Pool& P = *Pp;
    for (;;) {
        Job j;
        {
            std::unique_lock<std::mutex> lock(P.mu);
            P.cv_queue.wait(lock, [&] { return !P.queue.empty(); });
            j = P.queue.front();
            P.queue.pop_front();
        }
        if (j.flag)   // the records are home when the word behind their copy has arrived
            spin_until([&] { return *j.flag == j.want; });
        std::atomic_thread_fence(std::memory_order_acquire);
        const double t_ready = P.tracing ? std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - P.t0).count() : 0.0;
        if (P.error.load() == 0 && j.n_rec) {
            // (no helper is inside the previous piece's loops any more: the counters may be reset)
            spin_until([&] { return P.inside.load(std::memory_order_acquire) == 0; });
            P.cur = j;
            P.n_chunks = (uint32_t)((j.n_rec + CHUNK - 1) / CHUNK);
            if (P.chunk_off.size() < (size_t)P.n_chunks + 1) P.chunk_off.resize((size_t)P.n_chunks + 1);
            P.next_count.store(0);
            P.done_count.store(0);
            P.next_write.store(0);
            P.done_write.store(0);
            P.phase.store(1, std::memory_order_release);
            {
                std::lock_guard<std::mutex> lock(P.mu);
                ++P.job_seq;
            }
            P.cv_job.notify_all();
            run_phases(P, true);
            if (P.phase.load() == 2)
                spin_until([&] { return P.done_write.load(std::memory_order_acquire) >= P.n_chunks; });
            P.phase.store(0, std::memory_order_release);
            std::atomic_thread_fence(std::memory_order_seq_cst);
        }
        if (P.tracing)
            P.trace.push_back({t_ready, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - P.t0).count(), (double)j.n_rows});
        P.finished.fetch_add(1, std::memory_order_release);
    }
}

Pool* pool() {
    std::call_once(g_pool_once, [] {
        Pool* P = new Pool();
        // (a GPU box gives one GPU's process a share of the host's cores: the pool stays well inside it -- the caller's
        // thread and the HIP runtime's own threads need cores too, and threads beyond the share would stall everyone)
        unsigned n = cpu_share();
        // three quarters of what the process may use, 12 at most (measured at config 2 on a 16-CPU share: 4 threads 5.57 ms per
        // step, 7: 5.09, 10: 4.68, 12: 4.64; 14 leave the caller's thread and the runtime's threads without a CPU: 5.75)
        n = std::max(1u, std::min(n * 3 / 4, 12u));
        if (const char* e = getenv("PHASM_HOME_THREADS")) n = (unsigned)std::max(1, std::min(64, atoi(e)));
        try {
            P->thr.emplace_back(leader, P);
            P->thr.back().detach();   // (they sleep until the process ends)
            for (unsigned i = 1; i < n; ++i) {
                P->thr.emplace_back(helper, P);
                P->thr.back().detach();
            }
        } catch (const std::system_error&) {
        }
        if (P->thr.empty()) {
            delete P;
            P = nullptr;
        }
        g_pool = P;
    });
    return g_pool;
}

void begin(Pool* P, const uint32_t* len, uint32_t n_reads, bool tracing) {
    if (const char* e = getenv("PHASM_HOME_SPIN")) g_spin_limit.store((uint32_t)std::max(0, atoi(e)));
    else g_spin_limit.store(4096);
    P->len = len;
    P->n_reads = n_reads;
    P->error.store(0);
    P->submitted.store(0);
    P->finished.store(0);
    P->sum_l.store(0);
    P->sum_b.store(0);
    P->sum_e.store(0);
    P->tracing = tracing;
    P->trace.clear();
    P->t0 = std::chrono::steady_clock::now();
}

void submit(Pool* P, const Job& j) {
    {
        std::lock_guard<std::mutex> lock(P->mu);
        P->queue.push_back(j);
    }
    P->submitted.fetch_add(1, std::memory_order_release);
    P->cv_queue.notify_one();
}

void wait_all(Pool* P) {
    // (the caller has nothing else to do: it spins -- the last piece's rows are what the call is waiting for)
    spin_until([&] { return P->finished.load(std::memory_order_acquire) >= P->submitted.load(std::memory_order_acquire); });
}

}  // namespace home

po_status init_device(po_handle* h) {
    if (h->dev_ready) {
        HIP_TRY(h, hipSetDevice(h->device));
        return PO_OK;
    }
    AllocTrace tr("init_device", 0);
    const auto ti0 = std::chrono::steady_clock::now();
    auto imark = [&](const char* what) {
        if (tr.on) std::fprintf(stderr, "[init] %s at %.1f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ti0).count());
    };
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    imark("runtime up (hipGetDeviceCount)");
    if (e != hipSuccess || n == 0)
        return fail(h, PO_ERR_HIP, "no HIP device available (libphasm_overlap has no CPU fallback)");
    if (h->device < 0 || h->device >= n) return fail(h, PO_ERR_INVALID, "device ordinal out of range");
    HIP_TRY(h, hipSetDevice(h->device));
    hipDeviceProp_t prop;
    HIP_TRY(h, hipGetDeviceProperties(&prop, h->device));
    h->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    h->lds_max = prop.sharedMemPerBlock;
    if (const char* e = getenv("PHASM_POISON")) h->poison = (int)(strtol(e, nullptr, 0) & 0xFF);
    if (!getenv("PHASM_NO_KIT_POOL") && kit_take(h)) {
        h->ev = h->ev_sets[0];
        std::memset(h->pinned, 0, 1024);
        hipLaunchKernelGGL(po::k_fill_u32, dim3(1), dim3(64), 0, h->stream, reinterpret_cast<uint32_t*>(h->pinned_dev + 63), (uint64_t)1, 0u);
        (void)hipGetLastError();
        h->dev_ready = true;
        return PO_OK;
    }
    imark("device selected, properties read");
    HIP_TRY(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    imark("first stream made");
    for (int i = 0; i < 2 * EV_N; ++i) HIP_TRY(h, hipEventCreate(&h->ev_sets[i / EV_N][i % EV_N]));
    HIP_TRY(h, hipEventCreate(&h->ev_up0));
    HIP_TRY(h, hipEventCreate(&h->ev_up1));
    imark("first events made");
    HIP_TRY(h, hipHostMalloc(reinterpret_cast<void**>(&h->pinned), 1024, hipHostMallocDefault));   // 128 slots
    pin_note(h->pinned, 1024, 1u);
    HIP_TRY(h, hipHostGetDevicePointer(reinterpret_cast<void**>(&h->pinned_dev), h->pinned, 0));
    imark("landing zone made");
    if (const char* e = getenv("PHASM_POISON")) h->poison = (int)(strtol(e, nullptr, 0) & 0xFF);
    // the streams and events of the host-to-host call: created here (a few tenths of a millisecond each), not in its first call
    HIP_TRY(h, hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
    imark("copy stream made");
    HIP_TRY(h, hipStreamCreateWithFlags(&h->up_stream, hipStreamNonBlocking));
    HIP_TRY(h, hipStreamCreateWithFlags(&h->rc_stream, hipStreamNonBlocking));
    // (four streams = the runtime's four hardware queues, one each.  A fifth stream shares a queue with one of these, and
    // whatever it launches waits behind everything queued there -- rc_stream's kernels are all queued up front behind the
    // pieces' arrival events: profiles/r04_two_stream.txt.)
    imark("other streams made");
    for (int k = 0; k < PO_MAX_PIECES; ++k) {
        HIP_TRY(h, hipEventCreate(&h->ev_piece[k]));
        HIP_TRY(h, hipEventCreateWithFlags(&h->ev_rc[k], hipEventDisableTiming));
    }
    HIP_TRY(h, hipEventCreateWithFlags(&h->ev_first, hipEventDisableTiming));
    HIP_TRY(h, hipEventCreateWithFlags(&h->ev_meta, hipEventDisableTiming));
    imark("streams and events made");
    // the library's code object is loaded by the first launch out of it (15 ms in a fresh process): here, not in a call
    hipLaunchKernelGGL(po::k_fill_u32, dim3(1), dim3(64), 0, h->stream, reinterpret_cast<uint32_t*>(h->pinned_dev + 63), (uint64_t)1, 0u);
    (void)hipGetLastError();
    imark("first launch queued (code object loaded)");
    // ... and so are the hardware queues behind the three other streams and the runtime's copy paths: a stream's queue is made
    // by the first command it gets, the host->device / device->host machinery by the first copy in each direction -- 15 ms
    // of the first call of a process (`8 pieces queued at 15.056 ms`, tools/cold_probe.py) when left to the call.  One
    // word each way on the streams that will carry the copies, one launch on every stream; the device comes up while the
    // reads are still being added (result_pool_grow, po_add_fasta's warm-up thread), so none of this is waited for there.
    if (!getenv("PHASM_NO_WARM")) {
        void* w = nullptr;
        if (hipMalloc(&w, 256) == hipSuccess) {
            uint32_t* wd = static_cast<uint32_t*>(w);
            (void)hipMemcpyAsync(wd, h->pinned + 62, 8, hipMemcpyHostToDevice, h->up_stream);
            hipLaunchKernelGGL(po::k_fill_u32, dim3(1), dim3(64), 0, h->up_stream, wd + 8, (uint64_t)1, 0u);
            (void)hipMemcpyAsync(wd + 16, h->pinned + 62, 8, hipMemcpyHostToDevice, h->stream);
            hipLaunchKernelGGL(po::k_fill_u32, dim3(1), dim3(64), 0, h->rc_stream, wd + 24, (uint64_t)1, 0u);
            hipLaunchKernelGGL(po::k_fill_u32, dim3(1), dim3(64), 0, h->copy_stream, wd + 32, (uint64_t)1, 0u);
            (void)hipMemcpyAsync(h->pinned + 61, wd + 32, 8, hipMemcpyDeviceToHost, h->copy_stream);
            (void)hipMemcpyAsync(h->pinned + 60, wd + 16, 8, hipMemcpyDeviceToHost, h->stream);
            (void)hipStreamSynchronize(h->up_stream);
            (void)hipStreamSynchronize(h->rc_stream);
            (void)hipStreamSynchronize(h->copy_stream);
            (void)hipStreamSynchronize(h->stream);
            (void)hipFree(w);
        }
        (void)hipGetLastError();
        imark("queues and copy paths warmed");
        // every kernel of a 2-bit call is looked up in the code object now (the runtime resolves a kernel at its first launch:
        // ~35 of them at 0.1-0.3 ms each inside the first call otherwise)
        static const void* const warm_kernels[] = {
            (const void*)po::k_abs_woff, (const void*)po::k_build_tiles, (const void*)po::k_revcomp_store, (const void*)po::k_scatter_first,
            (const void*)po::k_paired_check, (const void*)po::k_call_init, (const void*)po::k_call_reset, (const void*)po::k_table_insert,
            (const void*)po::k_chain_fill, (const void*)po::k_chain_sort_short<uint32_t>, (const void*)po::k_chain_sort_long<uint32_t>,
            (const void*)po::k_table_finalize, (const void*)po::k_ps_reduce<uint32_t>, (const void*)po::k_ps_spine, (const void*)po::k_ps_down<uint32_t>,
            (const void*)po::k_ps_reduce<uint8_t>, (const void*)po::k_ps_down<uint8_t>, (const void*)po::k_ps_chain<uint32_t>,
            (const void*)po::k_ps_chain<uint8_t>, (const void*)po::k_ps_small,
            (const void*)po::k_scan_probe<2, true, true>, (const void*)po::k_scan_probe<2, true, false>, (const void*)po::k_scan_fixup<2, true>,
            (const void*)po::k_scan_fixup<2, false>, (const void*)po::k_scan_fill<2, true>, (const void*)po::k_scan_fill<2, false>,
            (const void*)po::k_read_label, (const void*)po::k_read_sort, (const void*)po::k_read_invert, (const void*)po::k_defer_split,
            (const void*)po::k_verify_a<2, false, true, true>, (const void*)po::k_verify_a<2, false, true, false>,
            (const void*)po::k_verify_a<2, true, true, false>, (const void*)po::k_select_local, (const void*)po::k_tile_rows<true>,
            (const void*)po::k_tile_rows<false>, (const void*)po::k_tail, (const void*)po::k_tail_cands, (const void*)po::k_select,
            (const void*)po::k_emit, (const void*)po::k_verify_flat, (const void*)po::k_deferred_rowcnt, (const void*)po::k_emit_cands,
            (const void*)po::k_wide_insert<2, 1>, (const void*)po::k_wide_insert<2, 16>, (const void*)po::k_wide_chain_fill<2, 1>,
            (const void*)po::k_wide_chain_fill<2, 16>, (const void*)po::k_wide_finalize<2, 1>, (const void*)po::k_wide_finalize<2, 16>,
            (const void*)po::k_chain_sort_short<uint64_t>, (const void*)po::k_chain_sort_long<uint64_t>,
            (const void*)po::k_wide_scan<2, false, true, 1>, (const void*)po::k_wide_scan<2, true, true, 1>,
            (const void*)po::k_wide_scan<2, false, false, 16>, (const void*)po::k_wide_scan<2, true, false, 16>};
        for (const void* k : warm_kernels) {
            hipFuncAttributes fa;
            (void)hipFuncGetAttributes(&fa, k);
        }
        (void)hipGetLastError();
        imark("kernels looked up");
    }
    h->dev_ready = true;
    return PO_OK;
}

// 2-bit code per byte; 0x80 = not one of upper-case A/C/G/T
struct BaseLut {
    uint8_t v[256];
    BaseLut() {
        std::memset(v, 0x80, sizeof(v));
        v[(unsigned char)'A'] = 0;
        v[(unsigned char)'C'] = 1;
        v[(unsigned char)'G'] = 2;
        v[(unsigned char)'T'] = 3;
    }
};
const BaseLut g_lut;

// Append one read to the packed store.  Layout: every read starts on a 16-byte boundary and is
// followed by at least one zero guard word (kernels read one word past the last data word).
// bits == 2: bytes other than upper-case A/C/G/T become exception records (code 0 in the packed
// words); returns false (and appends nothing) when they are too dense for that (> n/64 + 16), in
// which case the caller moves the whole handle to 8 bits per base.
bool append_packed(po_handle* h, const unsigned char* s, size_t n, int bits) {
    const size_t per = 64 / bits;
    WordStore& store = h->words[h->woff.size() & 1];  // (woff has one entry per read appended so far)
    const size_t old_size = store.size();
    const size_t off = (old_size + 1) & ~size_t(1);
    const size_t nw = (n + per - 1) / per;
    store.resize(off + nw + 1, 0);
    uint64_t* w = store.data() + off;
    if (bits == 2) {
        const uint8_t* lut = g_lut.v;
        uint8_t bad = 0;
        const size_t full = n / 32;
        for (size_t k = 0; k < full; ++k) {
            const unsigned char* q = s + k * 32;
            uint64_t acc = 0;
            for (int j = 0; j < 32; ++j) {
                const uint8_t c = lut[q[j]];
                bad |= c;
                acc |= (uint64_t)(c & 3) << (2 * j);
            }
            w[k] = acc;
        }
        if (full * 32 < n) {
            uint64_t acc = 0;
            for (size_t i = full * 32; i < n; ++i) {
                const uint8_t c = lut[s[i]];
                bad |= c;
                acc |= (uint64_t)(c & 3) << (2 * (i & 31));
            }
            w[full] = acc;
        }
        if (bad & 0x80) {
            size_t cnt = 0;
            for (size_t i = 0; i < n; ++i) cnt += lut[s[i]] >> 7;
            if (cnt > n / 64 + 16) {
                store.resize(old_size);
                return false;
            }
            for (size_t i = 0; i < n; ++i) {
                if (lut[s[i]] & 0x80) {
                    h->exc_pos.push_back((uint32_t)i);
                    h->exc_byte.push_back(s[i]);
                }
            }
        }
        h->exc_off.push_back((uint32_t)h->exc_pos.size());
    } else {
        for (size_t i = 0; i < n; ++i) w[i >> 3] |= (uint64_t)s[i] << ((i & 7) * 8);
    }
    h->woff.push_back(off);
    return true;
}

// The bytes of read r as they were added (2-bit mode: codes + exception records).
void materialize(const po_handle* h, size_t r, const WordStore* stores, const uint64_t* woff, std::vector<unsigned char>& out) {
    const uint32_t n = h->len[r];
    out.resize(n);
    const uint64_t* w = stores[r & 1].data() + woff[r];
    for (uint32_t i = 0; i < n; ++i) out[i] = "ACGT"[(w[i >> 5] >> ((i & 31) * 2)) & 3];
    for (uint32_t e = h->exc_off[r]; e < h->exc_off[r + 1]; ++e) out[h->exc_pos[e]] = h->exc_byte[e];
}

// Non-ACGT bytes too dense for exception records: re-encode everything held so far at 8 bits per
// base (lossless).
void widen_to_bytes(po_handle* h) {
    WordStore old_words[2];
    std::vector<uint64_t> old_off;
    old_words[0].swap(h->words[0]);
    old_words[1].swap(h->words[1]);
    old_off.swap(h->woff);
    std::vector<unsigned char> tmp;
    for (size_t r = 0; r < h->len.size(); ++r) {
        materialize(h, r, old_words, old_off.data(), tmp);
        append_packed(h, tmp.data(), h->len[r], 8);
    }
    h->bits = 8;
    h->all_pairs_rc = false;
    h->all_pairs_rcx = false;
    h->first_n = 0;
    h->first_words.clear();
    h->lead_n = 0;
    h->lead_words.clear();
    h->exc_off.assign(1, 0);
    h->exc_pos.clear();
    h->exc_byte.clear();
    h->pair_state.clear();
}

// IUPAC-aware complement, identity on everything else (the table of phasm_amd/io/fasta.py)
const unsigned char* comp_table() {
    static unsigned char comp[256];
    static bool init = false;
    if (!init) {
        for (int i = 0; i < 256; ++i) comp[i] = (unsigned char)i;
        const char* from = "ACGTURYKMBVDHSWNacgturykmbvdhswn";
        const char* to = "TGCAAYRMKVBHDSWNtgcaayrmkvbhdswn";
        for (int i = 0; from[i]; ++i) comp[(unsigned char)from[i]] = (unsigned char)to[i];
        init = true;
    }
    return comp;
}

// 2-bit mode, after read r (odd index) was appended: if it or its partner r-1 carries exception
// records, decide on the host whether the two are exact reverse complements of each other under a
// complement map that is an involution on the bytes present (the device check only sees 2-bit codes).
void host_pair_check(po_handle* h, size_t r, const unsigned char* s) {
    const size_t pair = r / 2;
    if (h->pair_state.size() <= pair) h->pair_state.resize(pair + 1, 0);
    const bool has_exc = h->exc_off[r - 1] != h->exc_off[r] || h->exc_off[r] != h->exc_off[r + 1];
    if (!has_exc) return;  // state 0: the device compares the codes
    const uint32_t n = h->len[r];
    uint8_t state = 1;
    if (h->len[r - 1] != n) {
        state = 2;
    } else {
        std::vector<unsigned char> prev;
        materialize(h, r - 1, h->words, h->woff.data(), prev);
        const unsigned char* c = comp_table();
        for (uint32_t i = 0; i < n; ++i) {
            const unsigned char x = prev[n - 1 - i], y = s[i];
            if (c[x] != y || c[y] != x) {
                state = 2;
                break;
            }
        }
    }
    h->pair_state[pair] = state;
}

// 2-bit mode, read r (odd index) just appended: are its packed words exactly the reverse complement of read r-1's?
// (word arithmetic of k_paired_check / k_revcomp_store on the host: ~2 us per 15 kb read)
bool packed_is_revcomp(const po_handle* h, size_t r) {
    const uint32_t L = h->len[r];
    if (h->len[r - 1] != L) return false;
    if (h->exc_off[r - 1] != h->exc_off[r] || h->exc_off[r] != h->exc_off[r + 1]) return false;  // exception records
    const uint64_t* R = h->words[0].data() + h->woff[r - 1];
    const uint64_t* S = h->words[1].data() + h->woff[r];
    const uint32_t nw = (L + 31) / 32;
    for (uint32_t w = 0; w < nw; ++w) {
        const int64_t o = (int64_t)L - 32 * (int64_t)w - 32;  // first base of R facing word w of S
        uint64_t x;
        uint32_t valid = 32;
        if (o >= 0) {
            const uint32_t sh = (uint32_t)(o & 31) * 2;
            x = sh ? (R[o >> 5] >> sh) | (R[(o >> 5) + 1] << (64 - sh)) : R[o >> 5];
        } else {
            valid = (uint32_t)(32 + o);
            x = R[0] << ((uint32_t)(-o) * 2);
        }
        uint64_t y = __builtin_bitreverse64(x);
        y = ((y >> 1) & 0x5555555555555555ull) | ((y & 0x5555555555555555ull) << 1);
        y = ~y;
        const uint64_t mask = valid >= 32 ? ~0ull : ((1ull << (valid * 2)) - 1ull);
        if (((y ^ S[w]) & mask) != 0) return false;
    }
    return true;
}

inline uint32_t cdiv(uint64_t a, uint32_t b) { return (uint32_t)((a + b - 1) / b); }

// first_words covers every read: the first two packed words of read r (a read owns its data words and a zero guard
// word; the word behind an EMPTY read is alignment padding, or -- for the last read of a store -- not part of the host
// store at all: zero on the device either way)
void note_first_words(po_handle* h) {
    const uint32_t n = (uint32_t)h->len.size();
    if (h->first_n == n && h->first_words.size() == 2 * (size_t)n) return;
    if (h->first_n > n || h->first_words.size() != 2 * (size_t)h->first_n) {
        h->first_n = 0;
        h->first_words.clear();
    }
    if (n - h->first_n > 1) h->first_words.reserve(2 * (size_t)n);   // (a bulk fill; one read at a time grows geometrically)
    for (uint32_t r = h->first_n; r < n; ++r) {
        const WordStore& store = h->words[r & 1];
        const uint64_t o = h->woff[r];
        h->first_words.push_back(o < store.size() ? store[o] : 0);
        h->first_words.push_back(o + 1 < store.size() ? store[o + 1] : 0);
    }
    h->first_n = n;
}

constexpr uint32_t LEAD_WORDS = 5;   // windows of 4 word-spaced K-mers at W phases: bases 0 .. 5 W - 2 of a read
void note_lead_words(po_handle* h) {
    const uint32_t n = (uint32_t)h->len.size();
    if (h->lead_n == n && h->lead_words.size() == (size_t)LEAD_WORDS * n) return;
    if (h->lead_n > n || h->lead_words.size() != (size_t)LEAD_WORDS * h->lead_n) {
        h->lead_n = 0;
        h->lead_words.clear();
    }
    h->lead_words.resize((size_t)LEAD_WORDS * n, 0);
    uint64_t* out = h->lead_words.data();
    for (uint32_t r = h->lead_n; r < n; ++r) {
        const WordStore& store = h->words[r & 1];
        const uint64_t o = h->woff[r];
        for (uint32_t k = 0; k < LEAD_WORDS; ++k) out[(size_t)r * LEAD_WORDS + k] = o + k < store.size() ? store[o + k] : 0;
    }
    h->lead_n = n;
}

// reads that can take part in an overlap of m bases or more
uint64_t count_eligible(po_handle* h, uint32_t m) {
    const uint64_t n = h->len.size();
    if (h->elig_n != n || h->elig_m != m) {
        uint64_t c = 0;
        for (uint64_t r = 0; r < n; ++r) c += h->len[r] >= m;
        h->elig_n = n;
        h->elig_m = m;
        h->elig_val = c;
    }
    return h->elig_val;
}

void shard_range(const po_handle* h, uint32_t shard, uint32_t nshards, uint32_t* r_begin, uint32_t* r_end, uint64_t* bases);

// words of host store 0 (the even reads) that belong to shard `shard` of `nshards`: [*begin, *begin + *count)
void store0_range(const po_handle* h, uint32_t shard, uint32_t nshards, uint64_t* begin, uint64_t* count) {
    uint32_t rb = 0, re = 0;
    shard_range(h, shard, nshards, &rb, &re, nullptr);
    const uint32_t n = (uint32_t)h->len.size();
    const uint32_t e0 = (rb + 1u) & ~1u, e1 = (re + 1u) & ~1u;   // first even read of this shard / of the next one
    const uint64_t w0 = e0 < n ? h->woff[e0] : h->words[0].size();
    const uint64_t w1 = e1 < n ? h->woff[e1] : h->words[0].size();
    *begin = w0;
    *count = w1 > w0 ? w1 - w0 : 0;
}

// part `part` of `nparts` of that range (equal chunks of an even number of words, the last one shorter or empty): the
// sharded upload is cut this way so that the host->device copy of one part runs under the all-gather of the part before
void store0_part_range(const po_handle* h, uint32_t shard, uint32_t nshards, uint32_t part, uint32_t nparts, uint64_t* begin, uint64_t* count) {
    uint64_t wb = 0, wc = 0;
    store0_range(h, shard, nshards, &wb, &wc);
    const uint64_t cs = (((wc + nparts - 1) / nparts) + 1) & ~uint64_t(1);
    const uint64_t lo = std::min(wc, (uint64_t)part * cs), hi = std::min(wc, (uint64_t)(part + 1) * cs);
    *begin = wb + lo;
    *count = hi - lo;
}

// Everything of an upload but the packed words themselves: scan tiles counted, device buffers sized, per-read
// offsets / lengths / tile numbers copied, tile records built on the device (they need no read data).
// a page-locked copy of `bytes` bytes at `src` (valid until the next upload starts), or `src` itself when the block is
// too small for it / the source is large
const void* staged(po_handle* h, const void* src, size_t bytes) {
    if (!bytes || bytes > STAGE_MAX || !h->stage_host.p) return src;
    const size_t off = (h->stage_used + 63) & ~size_t(63);
    if (off + bytes > h->stage_host.cap) return src;
    std::memcpy(static_cast<char*>(h->stage_host.p) + off, src, bytes);
    h->stage_used = off + bytes;
    return static_cast<const char*>(h->stage_host.p) + off;
}

po_status upload_meta(po_handle* h, bool* generate_out) {
    const uint32_t n = (uint32_t)h->len.size();
    const size_t per = 64 / h->bits;
    {
        // (every copy of the previous upload has completed: upload() and the streamed step end with a synchronisation)
        size_t need = 0;
        for (const WordStore& w : h->words)
            if (!store_is_pinned(w) && w.size() * 8 <= STAGE_MAX) need += w.size() * 8 + 64;
        if (h->bits == 2) need += ((size_t)n + 1) * 4 + h->exc_pos.size() * 5 + 192;
        need += n / 2 + 64;
        h->stage_used = 0;
        if (need > 256) PO_TRY(ensure_host(h, h->stage_host, need));
    }
    // tiles: 64 words each, never spanning reads.  The host only counts them (first tile of every read); the
    // 32-byte records are written on the device (k_build_tiles) instead of travelling over PCIe (25 MB at config 2).
    // Counted once per state of the read set, together with a page-locked copy of the per-read arrays (an async copy
    // out of a std::vector goes through the runtime's staging buffer, synchronously).
    if (h->meta_n != n || h->meta_bits != h->bits || !h->meta_host.p) {
        h->h_read_tile0.assign((size_t)n + 1, 0);
        h->max_len = 0;
        uint64_t nt = 0;
        for (uint32_t r = 0; r < n; ++r) {
            h->h_read_tile0[r] = (uint32_t)nt;
            h->max_len = std::max(h->max_len, h->len[r]);
            const size_t nw = (h->len[r] + per - 1) / per;
            nt += (nw + po::TILE_WORDS - 1) / po::TILE_WORDS;
            if (nt > 0x7FFFFF00ull / po::WAVE) return fail(h, PO_ERR_CAPACITY, "too many scan tiles");
        }
        h->h_read_tile0[n] = (uint32_t)nt;
        h->n_tiles = (uint32_t)nt;
        PO_TRY(ensure_host(h, h->meta_host, (size_t)n * 16 + 64));
        char* mh = static_cast<char*>(h->meta_host.p);
        if (n) {
            std::memcpy(mh, h->woff.data(), (size_t)n * 8);
            std::memcpy(mh + (size_t)n * 8, h->len.data(), (size_t)n * 4);
        }
        std::memcpy(mh + (size_t)n * 12, h->h_read_tile0.data(), ((size_t)n + 1) * 4);
        h->meta_n = n;
        h->meta_bits = h->bits;
    }
    const char* mh = static_cast<const char*>(h->meta_host.p);

    // Device buffer: [store 0 | store 1 | 72 zero words] (a scan tile may read 64+1 words past a read's start).
    // Only store 0 travels when every odd read is the reverse complement of its even partner: store 1 is then
    // rebuilt on the device, bit for bit what the host packed (k_revcomp_store).
    const uint64_t base1 = (h->words[0].size() + 1) & ~uint64_t(1);
    const uint64_t nwords = base1 + h->words[1].size() + 72;
    const bool generate = h->bits == 2 && n >= 2 && (n % 2) == 0 && h->all_pairs_rcx && !getenv("PHASM_FULL_UPLOAD");
    *generate_out = generate;
    h->base1 = base1;
    h->dev_words = nwords;
    PO_TRY(ensure(h, h->d_words, nwords * 8));
    PO_TRY(ensure(h, h->d_woff, ((size_t)n + 1) * 8));
    PO_TRY(ensure(h, h->d_len, ((size_t)n + 1) * 4));
    PO_TRY(ensure(h, h->d_tiles, ((size_t)h->n_tiles + 1) * sizeof(po::TileRec)));
    PO_TRY(ensure(h, h->d_read_tile0, ((size_t)n + 1) * 4));
    HIP_TRY(h, hipEventRecord(h->ev_up0, h->stream));
    uint64_t* dw = h->d_words.as<uint64_t>();
    // (the guard words between the reads are zeros in the host stores already: only the seam and the tail need clearing)
    HIP_TRY(h, hipMemsetAsync(dw + base1 + h->words[1].size(), 0, 72 * 8, h->stream));
    if (base1 != h->words[0].size()) HIP_TRY(h, hipMemsetAsync(dw + h->words[0].size(), 0, 8, h->stream));
    h->upload_bytes = 0;
    if (n) {
        HIP_TRY(h, hipMemcpyAsync(h->d_woff.p, mh, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(h->d_len.p, mh + (size_t)n * 8, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
        h->upload_bytes += (size_t)n * 12;
        // store-relative offsets -> offsets into the device buffer
        hipLaunchKernelGGL(po::k_abs_woff, dim3(cdiv(n, 256)), dim3(256), 0, h->stream, h->d_woff.as<uint64_t>(), n, base1);
    }
    HIP_TRY(h, hipMemcpyAsync(h->d_read_tile0.p, mh + (size_t)n * 12, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, h->stream));
    h->upload_bytes += ((size_t)n + 1) * 4;
    if (h->n_tiles) {
        hipLaunchKernelGGL(po::k_build_tiles, dim3(cdiv(h->n_tiles, 256)), dim3(256), 0, h->stream, h->d_woff.as<uint64_t>(),
                           h->d_len.as<uint32_t>(), h->d_read_tile0.as<uint32_t>(), n, h->n_tiles, h->d_tiles.as<po::TileRec>());
    }
    // exception records (2-bit mode only; usually none).  Up before anything that looks at the reads: the kernel that
    // rebuilds the odd reads on the device needs them, and so does every verify
    const size_t n_exc = h->bits == 2 ? h->exc_pos.size() : 0;
    if (n_exc) {
        PO_TRY(ensure(h, h->d_exc_off, ((size_t)n + 1) * 4));
        PO_TRY(ensure(h, h->d_exc_pos, n_exc * 4));
        PO_TRY(ensure(h, h->d_exc_byte, n_exc));
        HIP_TRY(h, hipMemcpyAsync(h->d_exc_off.p, staged(h, h->exc_off.data(), ((size_t)n + 1) * 4), ((size_t)n + 1) * 4, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(h->d_exc_pos.p, staged(h, h->exc_pos.data(), n_exc * 4), n_exc * 4, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(h->d_exc_byte.p, staged(h, h->exc_byte.data(), n_exc), n_exc, hipMemcpyHostToDevice, h->stream));
        h->upload_bytes += ((size_t)n + 1) * 4 + n_exc * 5;
    }
    h->n_exc_uploaded = n_exc;
    HIP_TRY(h, hipGetLastError());
    return PO_OK;
}

po_status upload(po_handle* h) {
    PO_TRY(init_device(h));
    if (!h->dirty) return PO_OK;
    const uint32_t n = (uint32_t)h->len.size();
    bool generate = false;
    PO_TRY(upload_meta(h, &generate));
    uint64_t* dw = h->d_words.as<uint64_t>();
    const uint64_t base1 = h->base1;
    if (h->asm_pieces) {
        // sharded upload: piece k = the store-0 words of shard k's reads, uploaded by rank k, gathered over xGMI
        if (!generate) return fail(h, PO_ERR_INVALID, "po_upload_assemble needs reads added as (x, reverse complement of x) pairs");
        // (layout of the gathered buffer: [part][shard][slot])
        for (uint32_t part = 0; part < h->asm_parts; ++part) {
            for (uint32_t k = 0; k < h->asm_n; ++k) {
                uint64_t wb = 0, wc = 0;
                store0_part_range(h, k, h->asm_n, part, h->asm_parts, &wb, &wc);
                if (wc > h->asm_slot_words) return fail(h, PO_ERR_INVALID, "po_upload_assemble: a piece is longer than the slot");
                if (wc) HIP_TRY(h, hipMemcpyAsync(dw + wb, h->asm_pieces + ((size_t)part * h->asm_n + k) * h->asm_slot_words, wc * 8,
                                                  hipMemcpyDeviceToDevice, h->stream));
            }
        }
    } else if (!h->words[0].empty()) {
        const void* src0 = store_is_pinned(h->words[0]) ? h->words[0].data() : staged(h, h->words[0].data(), h->words[0].size() * 8);
        HIP_TRY(h, hipMemcpyAsync(dw, src0, h->words[0].size() * 8, hipMemcpyHostToDevice, h->stream));
        h->upload_bytes += h->words[0].size() * 8;
    }
    if (!generate && !h->words[1].empty()) {
        const void* src1 = store_is_pinned(h->words[1]) ? h->words[1].data() : staged(h, h->words[1].data(), h->words[1].size() * 8);
        HIP_TRY(h, hipMemcpyAsync(dw + base1, src1, h->words[1].size() * 8, hipMemcpyHostToDevice, h->stream));
        h->upload_bytes += h->words[1].size() * 8;
    }
    if (generate) {
        hipLaunchKernelGGL(po::k_revcomp_store, dim3(cdiv((uint64_t)(n / 2) * 64, 256)), dim3(256), 0, h->stream, dw,
                           h->d_woff.as<uint64_t>(), h->d_len.as<uint32_t>(), 0u, n / 2,
                           h->n_exc_uploaded ? h->d_exc_off.as<uint32_t>() : nullptr, h->d_exc_pos.as<uint32_t>());
        if (getenv("PHASM_VERIFY_GENERATED") && !h->words[1].empty()) {
            // test mode: the host's own store 1 is uploaded next to the generated one and compared word by word
            DevBuf tmp;
            PO_TRY(ensure(h, tmp, h->words[1].size() * 8));
            PO_TRY(ensure(h, h->d_scalars, 128));
            HIP_TRY(h, hipMemsetAsync(h->d_scalars.p, 0, 64, h->stream));
            HIP_TRY(h, hipMemcpyAsync(tmp.p, h->words[1].data(), h->words[1].size() * 8, hipMemcpyHostToDevice, h->stream));
            hipLaunchKernelGGL(po::k_count_diff, dim3(1024), dim3(256), 0, h->stream, dw + base1, tmp.as<uint64_t>(),
                               (uint64_t)h->words[1].size(), h->d_scalars.as<unsigned long long>());
            HIP_TRY(h, hipMemcpyAsync(h->pinned, h->d_scalars.p, 8, hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(h, hipStreamSynchronize(h->stream));
            tmp.release();
            if (h->pinned[0] != 0)
                return fail(h, PO_ERR_HIP, "generated reverse-complement store differs from the host's in " +
                                               std::to_string(h->pinned[0]) + " words");
        }
    }
    HIP_TRY(h, hipGetLastError());
    const size_t n_exc = h->n_exc_uploaded;   // (exception records went up with the per-read tables, upload_meta)
    // strand pairing: decides whether po_overlaps may compute one member of each mirror pair
    h->paired = false;
    const bool mirror_ok = !getenv("PHASM_NO_MIRROR");
    const bool try_paired = h->bits == 2 && n >= 2 && (n % 2) == 0 && mirror_ok && !generate;
    if (generate && mirror_ok) h->paired = true;  // (checked word by word on the host as the reads arrived)
    if (try_paired) {
        PO_TRY(ensure(h, h->d_scalars, 128));
        HIP_TRY(h, hipMemsetAsync(h->d_scalars.p, 0, 64, h->stream));
        const uint8_t* pair_state = nullptr;
        if (n_exc) {  // pairs with exception records were compared byte-wise on the host
            h->pair_state.resize(n / 2, 0);
            PO_TRY(ensure(h, h->d_pair_state, n / 2));
            HIP_TRY(h, hipMemcpyAsync(h->d_pair_state.p, staged(h, h->pair_state.data(), n / 2), n / 2, hipMemcpyHostToDevice, h->stream));
            pair_state = h->d_pair_state.as<uint8_t>();
        }
        hipLaunchKernelGGL(po::k_paired_check, dim3(cdiv((uint64_t)(n / 2) * 64, 256)), dim3(256), 0, h->stream,
                           h->d_words.as<uint64_t>(), h->d_woff.as<uint64_t>(), h->d_len.as<uint32_t>(), n / 2, pair_state,
                           h->d_scalars.as<uint32_t>());
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(h->pinned, h->d_scalars.p, 8, hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(h, hipEventRecord(h->ev_up1, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (try_paired) h->paired = (uint32_t)h->pinned[0] == 0;
    float ms = 0;
    (void)hipEventElapsedTime(&ms, h->ev_up0, h->ev_up1);
    h->stats.ms_upload = ms;
    h->stats.upload_bytes = h->upload_bytes;
    ++h->upload_gen;
    h->dirty = false;
    return PO_OK;
}

// a-side shard: contiguous read ranges balanced by bases
void shard_range(const po_handle* h, uint32_t shard, uint32_t nshards, uint32_t* r_begin, uint32_t* r_end, uint64_t* bases) {
    const uint32_t n = (uint32_t)h->len.size();
    // (the running sum of the read lengths is kept on the handle: a step of an N-rank job asks for dozens of shard and
    // piece ranges, and 100 k additions each time were milliseconds of host time per step)
    std::vector<uint64_t>& cum = const_cast<po_handle*>(h)->cum_len;
    if (cum.size() != (size_t)n + 1) {
        size_t have = cum.empty() ? 0 : std::min(cum.size() - 1, (size_t)n);   // (reads are only ever appended)
        cum.resize((size_t)n + 1);
        if (have == 0) cum[0] = 0;
        for (size_t r = have; r < n; ++r) cum[r + 1] = cum[r] + h->len[r];
    }
    auto cut = [&](uint32_t s) -> uint32_t {
        if (s == 0) return 0;
        if (s >= nshards) return n;
        const uint64_t target = (uint64_t)((__uint128_t)cum[n] * s / nshards);
        return (uint32_t)(std::lower_bound(cum.begin(), cum.end(), target) - cum.begin());
    };
    *r_begin = cut(shard);
    *r_end = cut(shard + 1);
    if (*r_end < *r_begin) *r_end = *r_begin;
    if (bases) *bases = cum[*r_end] - cum[*r_begin];
}

// exclusive scan of n items (u8 or u32) -> u32 offsets; *total_host gets the grand total
// (a pinned slot: valid after the next hipStreamSynchronize)
// the state of the single-pass scans (kernels.hip.h, ChainState): zero when allocated, left zero by every launch
po_status chain_state(po_handle* h, uint32_t n_tiles, po::ChainState** out, hipStream_t on, bool streamed = false) {
    const size_t need = po::chain_state_bytes(n_tiles);
    if (need > h->d_chain_state.cap) {
        PO_TRY(ensure(h, h->d_chain_state, std::max<size_t>(need * 2, 1u << 16), 1.0, true, streamed));
        HIP_TRY(h, hipMemsetAsync(h->d_chain_state.p, 0, h->d_chain_state.cap, on));
    }
    *out = h->d_chain_state.as<po::ChainState>();
    return PO_OK;
}

template <typename T>
po_status prefix_sum(po_handle* h, const T* in, uint64_t n, uint32_t* out, volatile uint64_t* total_host,
                     const uint64_t* also_src = nullptr, volatile uint64_t* also_host = nullptr, const uint32_t* extra = nullptr,
                     hipStream_t on = nullptr, uint64_t* total_dev_at = nullptr, const OverlapArgs& a = OverlapArgs()) {
    *total_host = 0;
    if (n == 0) return PO_OK;
    const hipStream_t ps = on ? on : h->stream;
    const uint32_t nblocks = cdiv(n, po::PS_TILE);
    uint64_t* total_dev = total_dev_at ? total_dev_at : h->d_scalars.as<uint64_t>();
    uint64_t* total_mapped = h->pinned_dev + (const_cast<uint64_t*>(total_host) - h->pinned);   // the slot as the device sees it
    uint64_t* also_mapped = also_host ? h->pinned_dev + (const_cast<uint64_t*>(also_host) - h->pinned) : nullptr;
    if (nblocks <= 64 && !getenv("PHASM_PS_CLASSIC")) {
        // ONE launch: decoupled look-back (k_ps_chain); `extra` is added to the input on the way (u32 inputs).  Short
        // inputs only -- the tile counts of a piece or a shard: hundreds of tiles spinning on status words across the
        // XCDs are slower than three launches

        po::ChainState* cs = nullptr;
        PO_TRY(chain_state(h, nblocks, &cs, ps, a.streamed));
        hipLaunchKernelGGL(po::k_ps_chain<T>, dim3(nblocks), dim3(po::PS_BLOCK), 0, ps, const_cast<T*>(in), extra, n, out, cs,
                           nblocks, total_dev, total_mapped, also_src, also_mapped);
        HIP_TRY(h, hipGetLastError());
        return PO_OK;
    }
    if (extra) {   // (u32 inputs: add in place first, as a launch of its own)
        hipLaunchKernelGGL(po::k_add_extra, dim3(cdiv(n, 256)), dim3(256), 0, ps, const_cast<uint32_t*>(reinterpret_cast<const uint32_t*>(in)),
                           extra, 0u, (uint32_t)n);
    }
    PO_TRY(ensure_piece(h, h->d_ps_blocks, (size_t)nblocks * 8, a));
    uint64_t* blocks = h->d_ps_blocks.as<uint64_t>();
    hipLaunchKernelGGL(po::k_ps_reduce<T>, dim3(nblocks), dim3(po::PS_BLOCK), 0, ps, in, n, blocks);
    hipLaunchKernelGGL(po::k_ps_spine, dim3(1), dim3(1024), 0, ps, blocks, nblocks, total_dev, total_mapped, also_src, also_mapped);
    hipLaunchKernelGGL(po::k_ps_down<T>, dim3(nblocks), dim3(po::PS_BLOCK), 0, ps, in, n, blocks, out);
    HIP_TRY(h, hipGetLastError());
    return PO_OK;
}

// one-workgroup form for short u32 inputs (kernels.hip.h, k_ps_small); `extra` is added into `in` first, `also_src`
// (a device counter) lands in the pinned slot `also_host`
po_status prefix_sum_small(po_handle* h, uint32_t* in, const uint32_t* extra, uint32_t n, uint32_t* out, volatile uint64_t* total_host,
                           const uint64_t* also_src, volatile uint64_t* also_host, hipStream_t on = nullptr, uint64_t* total_dev_at = nullptr) {
    *total_host = 0;
    if (n == 0) return PO_OK;
    const hipStream_t ps = on ? on : h->stream;
    uint64_t* total_dev = total_dev_at ? total_dev_at : h->d_scalars.as<uint64_t>();
    uint64_t* total_mapped = h->pinned_dev + (const_cast<uint64_t*>(total_host) - h->pinned);
    uint64_t* also_mapped = also_host ? h->pinned_dev + (const_cast<uint64_t*>(also_host) - h->pinned) : nullptr;
    hipLaunchKernelGGL(po::k_ps_small, dim3(1), dim3(1024), 0, ps, in, extra, n, out, total_dev, total_mapped,
                       also_src, also_mapped);
    HIP_TRY(h, hipGetLastError());
    return PO_OK;
}

void stage_times(po_stats& S, hipEvent_t* ev, bool ver_timed, bool full, bool pairs = true) {
    if (!full && !pairs) {   // (a piece of a streamed step that recorded nothing but its end)
        S.ms_index = S.ms_scan_count = S.ms_scan_fill = S.ms_verify = S.ms_select = S.ms_emit = 0.f;
        S.ms_total = S.ms_scan_probe = S.ms_verify_kernel = 0.f;
        return;
    }
    if (!full) {
        S.ms_index = S.ms_scan_count = S.ms_scan_fill = S.ms_verify = S.ms_select = S.ms_emit = 0.f;
        (void)hipEventElapsedTime(&S.ms_total, ev[EV_START], ev[EV_EMIT]);
        (void)hipEventElapsedTime(&S.ms_scan_probe, ev[EV_PROBE0], ev[EV_PROBE1]);
        S.ms_verify_kernel = 0.f;
        if (ver_timed) (void)hipEventElapsedTime(&S.ms_verify_kernel, ev[EV_VER0], ev[EV_VER1]);
        return;
    }
    (void)hipEventElapsedTime(&S.ms_index, ev[EV_START], ev[EV_INDEX]);
    (void)hipEventElapsedTime(&S.ms_scan_count, ev[EV_INDEX], ev[EV_COUNT]);
    (void)hipEventElapsedTime(&S.ms_scan_fill, ev[EV_COUNT], ev[EV_FILL]);
    (void)hipEventElapsedTime(&S.ms_verify, ev[EV_FILL], ev[EV_VERIFY]);
    (void)hipEventElapsedTime(&S.ms_select, ev[EV_VERIFY], ev[EV_SELECT]);
    (void)hipEventElapsedTime(&S.ms_emit, ev[EV_SELECT], ev[EV_EMIT]);
    (void)hipEventElapsedTime(&S.ms_total, ev[EV_START], ev[EV_EMIT]);
    (void)hipEventElapsedTime(&S.ms_scan_probe, ev[EV_PROBE0], ev[EV_PROBE1]);
    S.ms_verify_kernel = 0.f;
    if (ver_timed) (void)hipEventElapsedTime(&S.ms_verify_kernel, ev[EV_VER0], ev[EV_VER1]);
}

// The closing numbers of a call, or of a pending piece of a streamed step, once the stream behind them has been
// synchronised: the row count (pinned[rows_at]; rows_at < 0: there were no candidates, nothing was written there) and the
// four emit counters (pinned[cnt_at ..]), then the stage times.  Returns the row count.
uint64_t close_stats(po_handle* h, po_stats& S, int rows_at, int cnt_at, hipEvent_t* ev, bool ver_timed, bool full, bool pairs) {
    const uint64_t n_rows = rows_at < 0 ? 0 : h->pinned[rows_at];
    S.n_rows = n_rows;
    S.n_verified = h->pinned[cnt_at];
    S.sum_overlap_bases = h->pinned[cnt_at + 1];
    S.verify_bytes_algo = h->pinned[cnt_at + 2];
    S.verify_bytes_exec = h->pinned[cnt_at + 3];
    stage_times(S, ev, ver_timed, full, pairs);
    return n_rows;
}

// the closing part of run_overlaps for a pending piece of a streamed step; the handle's stream has been synchronised
// since the piece was queued.  Returns the piece's row count.
// *needs_classic: k_tail found reads handed to the global (a, b) table and wrote nothing (the piece's workspaces have
// been reused by now: the streamed step gives up and the call takes the chunked form).
uint64_t finish_piece(po_handle* h, bool* needs_classic) {
    po_handle::Pending& P = h->st_pend;
    *needs_classic = P.tail && h->pinned[P.zone + 7] != 0;
    if (P.cap_c) {   // the count that was predicted: more than the buffers held -> nothing was computed
        P.S.n_candidates = h->pinned[P.zone + 8];
        if (P.S.n_candidates > P.cap_c) *needs_classic = true;
    }
    P.valid = false;
    return close_stats(h, P.S, P.tail ? P.zone : 2, P.tail ? P.zone + 1 : 4, P.ev, P.ver_timed, P.full_events, P.pair_events);
}

// The PHASM_* switches of run_overlaps, read once per call: plan() and index_flavour() decide from them before anything is
// launched, the stages see what was decided.
struct OverlapSwitches {
    const char* index = getenv("PHASM_INDEX");                  // wide | narrow
    const char* wide_window = getenv("PHASM_WIDE_WINDOW");      // 1 | 4 | 16: a smaller window than min_length allows (tests, A/B)
    const char* table_mult = getenv("PHASM_TABLE_MULT");
    const char* scan_waves = getenv("PHASM_SCAN_WAVES");
    const char* pred_scale = getenv("PHASM_PRED_SCALE");        // (tests: a prediction that is too small)
    const char* verify_order = getenv("PHASM_VERIFY_ORDER");
    const char* verify_staged = getenv("PHASM_VERIFY_STAGED");  // 0: candidate records not staged in LDS
    const char* dp_kernel = getenv("PHASM_DP_KERNEL");          // bits | lanes | wave
    const char* dp_kernel_soft = getenv("PHASM_DP_KERNEL_SOFT");  // (tests: "lanes" where a lane mapping applies at all, no error elsewhere)
    const char* dp_sort = getenv("PHASM_DP_SORT");              // (tests force it on small inputs)
    const bool no_index_reuse = getenv("PHASM_NO_INDEX_REUSE") != nullptr;
    const bool debug_left = getenv("PHASM_DEBUG_LEFT") != nullptr;   // how many positions did the scan waves defer to k_scan_fixup?
    const bool piece_reset = getenv("PHASM_PIECE_RESET") != nullptr;
    const bool sync_count = getenv("PHASM_SYNC_COUNT") != nullptr;
    const bool tail_classic = getenv("PHASM_TAIL_CLASSIC") != nullptr;
    const bool select_kernel = getenv("PHASM_SELECT_KERNEL") != nullptr;   // the separate k_select_local launch (tests compare)
    const bool compact_sync = getenv("PHASM_COMPACT_SYNC") != nullptr;
    const int phase_events = phase_events_env();
};

// ---- index flavour.  narrow: prefix K-mer per read + LDS filter + every position probed (best up
// to ~150 k reads: the filter needs ~10 bits per read in 128 KB of LDS).  wide: W K-mers per read,
// only word-aligned K-mers of a probed, no filter (linear in the input; needs min_length >= 2W-1).
// ww: window of the wide index's minimiser scheme (kernels.hip.h WideEnc) -- the largest of 16 / 4 / 1 words with
// W ww + W - 1 <= min_length.  A streamed step's index is built from the `lead` words of every read that travel ahead of
// the pieces: two, or five (LEAD_WORDS, windows of 4).  overlaps_streamed asks with lead = LEAD_WORDS to learn whether five
// are worth sending, run_overlaps with what was sent.
struct IndexFlavour {
    bool wide;
    uint32_t ww;
};
// inexact (po_overlaps_ex with max_diff > 0): always narrow.  That mode is DEFINED on the narrow index's anchors -- b's prefix
// K-mer at a[p..p+K) (extend.hip.h) -- and the wide index finds a pair through another K-mer of b, the one at offset (-p) mod W
// (or a window minimiser further in) facing a word of a: the same candidates only while every base up to there matches.  With
// differences it would miss anchors whose first difference lies before that K-mer's end and list others whose prefix K-mer
// is not intact (tests/test_gpu_extend_edges.py: two anchors of one pair, the longer one 2 bases out of phase).
IndexFlavour index_flavour(po_handle* h, uint32_t m, bool streamed, uint32_t lead, const OverlapSwitches& sw, bool inexact = false) {
    const uint32_t W = 64 / h->bits;
    bool wide = count_eligible(h, m) > 160000 && m >= 2 * W - 1;
    if (sw.index) {
        if (!strcmp(sw.index, "wide")) wide = m >= 2 * W - 1;
        if (!strcmp(sw.index, "narrow")) wide = false;
    }
    if (inexact) wide = false;
    uint32_t ww = 1;
    if (wide && h->bits == 2) {
        ww = m >= W * 16 + W - 1 ? 16u : m >= W * 4 + W - 1 ? 4u : 1u;
        if (streamed) ww = (ww >= 4 && lead >= LEAD_WORDS) ? 4u : 1u;
        if (sw.wide_window) {
            const uint32_t v = (uint32_t)atoi(sw.wide_window);
            if ((v == 1 || v == 4 || v == 16) && v <= ww) ww = v;
        }
    }
    return {wide, ww};
}

// the row buffer of a result: the one kept from an earlier call where it is large enough (rows_late: it holds worst_rows,
// the rows are written before their number has reached the host), else a new one for n_rows -- with room for the worst
// case up to 2 GiB, so that the next call of this size need not ask
po_status take_row_buffer(po_handle* h, po_result* res, bool rows_late, uint64_t n_rows, uint64_t worst_rows, bool streamed = false) {
    if (rows_late || (h->spare_rows.cap >= n_rows * sizeof(po_row) && h->spare_rows.p)) {
        res->d_rows = h->spare_rows;
        h->spare_rows = DevBuf();
    } else {
        h->spare_rows.release();
    }
    if (rows_late) return PO_OK;
    const size_t exact = n_rows * sizeof(po_row);
    size_t roomy = worst_rows * sizeof(po_row) <= (2ull << 30) ? (size_t)(worst_rows * sizeof(po_row)) : 0;
    if (roomy && streamed) roomy += 4096 * sizeof(po_row);   // (room for the next call's predicted count and its slack)
    return ensure(h, res->d_rows, std::max<size_t>(std::max(exact, roomy), 256), 1.0, false, streamed);
}

// One run_overlaps call: what plan() decided, the workspaces, and what each stage leaves for the stages behind it.
// A stage may read the arguments, the plan and what earlier stages wrote here; it reads no environment.  On the handle
// it uses the device buffers, the landing zone and the streams, and it writes only what outlives the call: the idx_* cache,
// sl_*, st_pend / st_selfclean, the kept buffers and the statistics.
template <int BITS>
struct OverlapCall {
    static constexpr uint32_t W = 64 / BITS;
    po_handle* const h;
    const OverlapArgs& a;
    po_result* const res;
    const OverlapSwitches sw;
    const hipStream_t st;
    po_stats& S;

    // ---- plan(): decided before anything is launched
    uint32_t n = 0, m = 1, K = 1;
    uint64_t kmask = 0;
    // strand-mirror mode + the read order that picks the canonical member of a mirror pair (keep_bits):
    // 1 = index order (whole-set calls), 2 = scrambled block order (sharded calls, balances verify work)
    // (inexact extension: every candidate is extended itself, no strand-mirror shortcut)
    // 3 = reversed index order, a piece of a streamed step (kernels.hip.h, mirror_rank): the scan keeps containment
    // candidates of any b, the verify kernel only those whose b has arrived (b < a.r_end)
    uint32_t paired = 0, paired_ver = 0, dpE = 0, dpW = 0;
    uint32_t r_begin = 0, r_end = 0, tile_begin = 0, tile_end = 0, ntiles = 0;
    uint64_t n_elig = 0;
    bool wide = false;
    uint32_t ww = 1;
    bool slice_build = false;   // build one sub-table of the sliced wide index, then stop
    bool ext_idx = false;       // probe a gathered sliced index
    bool own_lists = false;     // duplicates are settled inside each read's own candidate list (k_select_local), see build_index
    uint32_t tbits = 10, nslots = 0, bloom_log2 = 13;
    size_t bloom_bytes = 0, n_entries = 0, chain_elem = 4;
    bool phase_events = true;   // this call records the stage-boundary events (phase_events_env)
    bool pair_events = true;    // ... at least the pairs around the two big kernels and the call's start / end
    bool reuse_index = false, fold_clear = false;
    uint32_t scan_waves = 0, scan_grid = 0;
    bool self_clean = false;    // a piece of a streamed step that leaves the per-call counters zero for the next piece
    bool sel_in_verify = false, staged = false, dp_lanes = false, dp_bitvec = false;
    int zone = 64;              // this piece's slots of the pinned landing area

    // ---- workspaces()
    const uint64_t* words = nullptr;
    const uint64_t* woff = nullptr;
    const uint32_t* len = nullptr;
    po::Slot* table = nullptr;
    uint32_t *slot_cnt = nullptr, *slot_cur = nullptr, *slot_start = nullptr, *read_slot = nullptr, *chain = nullptr;
    uint32_t *bloom = nullptr, *selfrep = nullptr, *tile_off_p = nullptr, *n_long = nullptr;
    unsigned long long* scalars = nullptr;   // [0] scan total, [1] n_long, [3] rows, [4..7] emit counters
    uint32_t* n_deferred = nullptr;          // reads k_select_local hands to the global table

    // ---- the stages' results
    po::ScanArgs A = {};
    po::WideArgs WA = {};
    uint32_t cap_c = 0;
    bool async_count = false, pred_order = true;
    po::CandGuard G = {nullptr, 0u};
    uint64_t n_cand64 = 0, worst_rows = 0;
    uint32_t n_cand = 0, n_selfrep_reads = 0;
    bool use_order = false, defer_needed = false;
    bool ver_timed = false;     // the verify kernel ran (there were candidates): its own events are valid
    bool compact_tail = false, can_tail = false;
    bool rows_late = false;     // rows emitted into a kept buffer before their number reached the host
    bool cands_late = false, cands_ext = false;  // the same for compacted candidates (want_cands): destination chosen before the number was known
    uint64_t cands_cap = 0;
    bool used_tail = false;     // the call's tail ran as k_tail (counts in pinned[tail_zone..], fallback flag in pinned[tail_zone + 7])
    int tail_zone = 48;

    OverlapCall(po_handle* h_, const OverlapArgs& a_, po_result* res_) : h(h_), a(a_), res(res_), st(h_->stream), S(h_->stats) {}

    // a workspace of this call; ws_piece: one whose size follows the candidate count of the a-side range at hand
    po_status ws(DevBuf& b, size_t bytes, bool arena_ok = true) { return ensure(h, b, bytes, 1.0, arena_ok, a.streamed); }
    po_status ws_piece(DevBuf& b, size_t bytes) { return ensure_piece(h, b, bytes, a); }
    template <typename T>
    po_status prefix(const T* in, uint64_t count, uint32_t* out, volatile uint64_t* total_host) {
        return prefix_sum<T>(h, in, count, out, total_host, nullptr, nullptr, nullptr, nullptr, nullptr, a);
    }

    // *done: the call has nothing (more) to do
    po_status plan(bool* done) {
        *done = true;
        n = (uint32_t)h->len.size();
        m = a.min_length ? a.min_length : 1;  // a suffix array has no empty suffix
        K = m < W ? m : W;
        kmask = K * BITS >= 64 ? ~0ull : ((1ull << (K * BITS)) - 1ull);
        const float keep_upload = S.ms_upload;
        S = po_stats();
        S.ms_upload = keep_upload;
        S.upload_bytes = h->upload_bytes;
        S.bits_per_base = BITS;
        S.kmer = K;
        S.n_reads = n;
        S.total_bases = h->total_bases;
        dpE = a.dp ? a.dp_E : 0u;
        dpW = a.dp && a.dp_E ? a.dp_W : 0u;
        paired = (BITS == 2 && h->paired && dpE == 0) ? (a.streamed ? po::PAIRED_STREAM_ALL : a.nshards > 1 ? 2u : 1u) : 0u;
        paired_ver = a.streamed ? po::paired_stream(a.r_end) : paired;
        if (a.streamed && (!paired || a.want_cands)) return fail(h, PO_ERR_INVALID, "streamed step without strand pairs");
        S.paired = paired ? 1u : 0u;
        S.max_diff = dpE;
        S.band = dpW;
        if (a.dp && dpE && a.want_cands) return fail(h, PO_ERR_INVALID, "the candidate (multi-GPU) form has no inexact mode");
        if (a.dp && dpE && BITS == 2 && !h->exc_pos.empty())
            return fail(h, PO_ERR_INVALID, "po_overlaps_ex with max_diff > 0 needs pure upper-case ACGT reads (or the 8-bit representation)");

        r_end = n;
        S.shard_bases = h->total_bases;
        if (a.streamed) {
            r_begin = a.r_begin;
            r_end = a.r_end;
            S.shard_bases = 0;
            for (uint32_t r = r_begin; r < r_end; ++r) S.shard_bases += h->len[r];
        } else if (a.nshards > 1) {
            shard_range(h, a.shard, a.nshards, &r_begin, &r_end, &S.shard_bases);
        }
        tile_begin = h->h_read_tile0[r_begin];
        tile_end = h->h_read_tile0[r_end];
        ntiles = tile_end - tile_begin;
        S.n_tiles = ntiles;

        n_elig = count_eligible(h, m);
        S.n_eligible = n_elig;
        res->count = 0;
        if (n == 0 || n_elig == 0 || ntiles == 0) return PO_OK;

        const IndexFlavour f = index_flavour(h, m, a.streamed, h->st_lead, sw, dpE != 0);
        wide = f.wide;
        ww = f.ww;
        S.wide_index = wide ? 1u : 0u;
        slice_build = a.build_n > 1;
        ext_idx = a.ext_index != nullptr;
        if (slice_build) {
            h->sl_is_wide = wide;
            if (!wide) return PO_OK;                    // (the narrow index is 0.06 ms: every rank builds its own)
        }
        if (ext_idx && !wide) return fail(h, PO_ERR_INVALID, "a sliced index was supplied, but this call uses the narrow index");
        own_lists = a.nshards > 1 || a.streamed || wide;
        uint64_t n_keys = wide ? n_elig * W : n_elig;
        if (slice_build) n_keys = n_keys / a.build_n + n_keys / (16ull * a.build_n) + 4096;  // (a slice's share + slack)
        // ---- sizes
        // narrow: 5-10 slots per key, probed in aligned groups of four (kernels.hip.h PROBE_GROUP).  A probe for an
        // absent key needs more than its group when all four slots are taken: 0.75 % of the groups at 5.2 slots per
        // key (7 % at 2.6), and those positions go to the leftover list; 8 MB at config 2
        double table_mult = wide ? 2.0 : 5.0;
        if (sw.table_mult) table_mult = std::max(wide ? 2.0 : 1.5, atof(sw.table_mult));
        if (slice_build) table_mult = 1.5;   // (a sub-table travels over xGMI: the smallest power of two that keeps the load <= 2/3)
        while ((double)(1ull << tbits) < table_mult * (double)n_keys) ++tbits;
        if (ext_idx) tbits = a.ext_tbits;
        if (tbits > 30) return fail(h, PO_ERR_CAPACITY, "too many reads for the anchor table");
        // (+1: the slot of the all-ones key; narrow: three more so that a group fetch of that slot stays in bounds)
        nslots = (1u << tbits) + (wide ? 1u : po::PROBE_GROUP);
        while (bloom_log2 < 20 && (1ull << bloom_log2) < 16 * n_elig) ++bloom_log2;
        bloom_bytes = (size_t)1 << (bloom_log2 - 3);
        n_entries = wide ? (size_t)n * W : (size_t)n;     // index entries (slots of read_slot / chain)
        chain_elem = wide ? 8 : 4;

        phase_events = sw.phase_events >= 0 ? sw.phase_events == 1 : !a.streamed;
        pair_events = phase_events || sw.phase_events == 2 || (sw.phase_events < 0 && !a.streamed);
        // the index THIS handle built for exactly this device copy of the reads (same upload, min_length, flavour, size)
        reuse_index = !slice_build && !ext_idx && h->idx_valid && h->idx_gen == h->upload_gen && h->idx_m == m &&
                      h->idx_wide == wide && h->idx_tbits == tbits && h->idx_bits == (uint32_t)BITS && h->idx_ww == ww && h->poison < 0 &&
                      !sw.no_index_reuse;
        // (narrow scan on a reused index: the reset kernel also clears the scan's two small per-call arrays, scan_count)
        fold_clear = reuse_index && !wide;
        scan_waves = po::SCAN_BLOCK / 64;
        if (sw.scan_waves) scan_waves = std::max(1, std::min(16, atoi(sw.scan_waves)));
        scan_grid = std::max<uint32_t>(1, std::min<uint32_t>((uint32_t)h->n_cu, cdiv(ntiles, scan_waves)));
        // (the pieces of a streamed step clean up after themselves -- k_scan_fixup zeroes its list counters, the fused tail its
        // counters, the first piece's reset clears tile_extra for every tile of the read set --: no reset launch per piece)
        self_clean = !wide && a.streamed && !sw.debug_left && !sw.piece_reset;
        zone = 64 + 16 * (int)(a.shard & 1u);
        // the longest-only selection inside each read's list runs in the verify kernel's epilogue where the exact verify runs
        // (not the DP kernels, which have no per-read workgroup); PHASM_SELECT_KERNEL=1 keeps the separate launch
        sel_in_verify = own_lists && !a.dp && !sw.select_kernel;
        // candidate records staged in LDS (word offsets must fit 32 bits); PHASM_VERIFY_STAGED=0 switches back
        staged = h->dev_words < 0xFFFFFFF0ull;
        if (sw.verify_staged) staged = staged && atoi(sw.verify_staged) != 0;
        if (a.dp) {
            // three mappings of the same DP (extend.hip.h), same rows bit for bit: a LANE per candidate with the band row as a
            // BIT VECTOR (k_extend_bits: 2-bit reads, band <= 15 -- the default where it applies), a lane per candidate with
            // the band row in registers (k_extend_lanes), a WAVE per candidate with a lane per diagonal (k_extend_dp: any
            // encoding, band <= 30).  PHASM_DP_KERNEL=bits|lanes|wave forces one (the tests run all three)
            dp_lanes = dp_bitvec = BITS == 2 && dpW <= 15;
            if (sw.dp_kernel) {
                if (!strcmp(sw.dp_kernel, "wave")) dp_lanes = dp_bitvec = false;
                if (!strcmp(sw.dp_kernel, "lanes")) dp_bitvec = false;
                if ((!strcmp(sw.dp_kernel, "lanes") || !strcmp(sw.dp_kernel, "bits")) && !(BITS == 2 && dpW <= 15))
                    return fail(h, PO_ERR_INVALID, "PHASM_DP_KERNEL=lanes|bits needs 2-bit reads and band <= 15");
            }
            if (sw.dp_kernel_soft && !strcmp(sw.dp_kernel_soft, "lanes")) dp_bitvec = false;
        }
        *done = false;
        return PO_OK;
    }

    po_status workspaces() {
        PO_TRY(ws(h->d_scalars, 128));
        if (!ext_idx) {   // (a supplied index needs none of the build's workspaces)
            PO_TRY(ws(h->d_table, (size_t)nslots * sizeof(po::Slot)));
            PO_TRY(ws(h->d_slot_cnt, (size_t)nslots * 4));
            PO_TRY(ws(h->d_slot_cur, (size_t)nslots * 4));
            PO_TRY(ws(h->d_slot_start, ((size_t)nslots + 1) * 4));
            PO_TRY(ws(h->d_read_slot, n_entries * 4));
            // a slice's chain holds its share of the entries (+ slack; the exact number comes back from the prefix sum)
            const size_t chain_entries = slice_build ? n_entries / a.build_n + n_entries / (4ull * a.build_n) + 65536 : n_entries;
            PO_TRY(ws(h->d_chain, std::min(chain_entries, n_entries) * chain_elem));
            PO_TRY(ws(h->d_chain_tmp, std::min(chain_entries, n_entries) * chain_elem));
            PO_TRY(ws(h->d_long_list, (size_t)nslots * 4));
            if (wide) PO_TRY(ws(h->d_entry_off, n_entries * 2));
        }
        PO_TRY(ws(h->d_bloom, bloom_bytes));
        PO_TRY(ws(h->d_selfrep, (size_t)n * 4));
        PO_TRY(ws(h->d_tile_count, ((size_t)h->n_tiles + 1) * 4));
        PO_TRY(ws(h->d_tile_off, ((size_t)h->n_tiles + 2) * 4 * 2));   // (twice: the pieces of a streamed step alternate)
        PO_TRY(ws(h->d_truemask, ((size_t)h->n_tiles + 1) * po::WAVE * 4));

        words = h->d_words.as<uint64_t>();
        woff = h->d_woff.as<uint64_t>();
        len = h->d_len.as<uint32_t>();
        table = h->d_table.as<po::Slot>();
        slot_cnt = h->d_slot_cnt.as<uint32_t>();
        slot_cur = h->d_slot_cur.as<uint32_t>();
        slot_start = h->d_slot_start.as<uint32_t>();
        read_slot = h->d_read_slot.as<uint32_t>();
        chain = h->d_chain.as<uint32_t>();
        bloom = h->d_bloom.as<uint32_t>();
        selfrep = h->d_selfrep.as<uint32_t>();
        // the small per-piece state (candidate count, emit counters, tile offsets) exists twice, by the piece's parity, like the
        // piece's slots of the landing zone (`zone`)
        const uint32_t parity = a.streamed ? (a.shard & 1u) : 0u;
        scalars = h->d_scalars.as<unsigned long long>() + 8 * parity;
        tile_off_p = h->d_tile_off.as<uint32_t>() + (size_t)parity * ((size_t)h->n_tiles + 2);
        n_long = reinterpret_cast<uint32_t*>(scalars + 1);
        n_deferred = reinterpret_cast<uint32_t*>(scalars + 1) + 1;

        if (h->poison >= 0) {
            // PHASM_POISON: whatever earlier calls left in the per-call workspaces is replaced by the caller's byte
            DevBuf* all[] = {&h->d_table, &h->d_slot_cnt, &h->d_slot_cur, &h->d_slot_start, &h->d_read_slot, &h->d_chain,
                             &h->d_chain_tmp, &h->d_long_list, &h->d_bloom, &h->d_selfrep, &h->d_tile_count, &h->d_tile_off,
                             &h->d_truemask, &h->d_ps_blocks, &h->d_left, &h->d_left_cnt, &h->d_tile_extra, &h->d_cand_a,
                             &h->d_cand_p, &h->d_cand_b, &h->d_type, &h->d_rowcnt, &h->d_row_off, &h->d_flag, &h->d_pair_key,
                             &h->d_vlabel, &h->d_vrank, &h->d_vperm, &h->spare_rows, &h->spare_cands};
            for (DevBuf* b : all)
                if (b->p) HIP_TRY(h, hipMemsetAsync(b->p, h->poison, b->cap, st));
        }
        return PO_OK;
    }

    // every chain sorted by the order the scan walks it in: short ones in place, the long ones listed for k_chain_sort_long
    template <typename T>
    void sort_chains() {
        hipLaunchKernelGGL(po::k_chain_sort_short<T>, dim3(cdiv(nslots, 256)), dim3(256), 0, st, slot_cnt, slot_start,
                           nslots, h->d_chain.as<T>(), h->d_long_list.as<uint32_t>(), n_long);
        hipLaunchKernelGGL(po::k_chain_sort_long<T>, dim3(64), dim3(256), 0, st, slot_cnt, slot_start,
                           h->d_long_list.as<uint32_t>(), n_long, h->d_chain.as<T>(), h->d_chain_tmp.as<T>());
    }

    // ---- index: anchor table, chains, Bloom filter.  Built per call like the reference builds its suffix array per
    // call (overlapper.cpp:33-36) -- unless THIS handle built exactly this index for exactly this device copy of the
    // reads already (reuse_index): the chunks of po_overlaps_to_host and the shards of a multi-GPU step then share one
    // build instead of repeating it (the replicated part of a sharded step).
    // *done: a slice build or the index-only pass of a streamed step, which end here
    po_status build_index(bool* done) {
        *done = true;
        if (pair_events) HIP_TRY(h, hipEventRecord(h->ev[EV_START], st));
        S.index_reused = reuse_index ? 1u : 0u;
        h->idx_valid = false;
        if (fold_clear) {
        } else if (reuse_index || ext_idx) {
            hipLaunchKernelGGL(po::k_call_reset, dim3(cdiv(std::max(n, 16u), 256)), dim3(256), 0, st, selfrep, n, scalars, 8u,
                               (uint32_t*)nullptr, 0u, (uint32_t*)nullptr, 0u);
        } else {
            const uint32_t bloom_words = (uint32_t)(bloom_bytes / 4);
            const uint32_t init_n = std::max(std::max(nslots, n), std::max(bloom_words, 8u));
            hipLaunchKernelGGL(po::k_call_init, dim3(cdiv(init_n, 256)), dim3(256), 0, st, table, nslots, slot_cnt, slot_cur, selfrep, n,
                               bloom, bloom_words, h->d_scalars.as<unsigned long long>());
        }
        if (reuse_index || ext_idx) {
            // (nothing to build)
        } else if (!wide) {
            hipLaunchKernelGGL(po::k_table_insert, dim3(cdiv(n, 256)), dim3(256), 0, st, words, woff, len, n, m, kmask, table,
                               tbits, slot_cnt, read_slot, bloom, bloom_log2, (uint32_t)BITS);
            PO_TRY(prefix<uint32_t>(slot_cnt, nslots, slot_start, &h->pinned[0]));
            hipLaunchKernelGGL(po::k_chain_fill, dim3(cdiv(n, 256)), dim3(256), 0, st, read_slot, n, slot_start, slot_cur, chain);
            sort_chains<uint32_t>();
            hipLaunchKernelGGL(po::k_table_finalize, dim3(cdiv(nslots, 256)), dim3(256), 0, st, table, nslots, slot_cnt,
                               slot_start, chain, len);
        } else {
            uint16_t* entry_off = h->d_entry_off.as<uint16_t>();
            auto k_ins = ww == 16 ? po::k_wide_insert<BITS, 16> : ww == 4 ? po::k_wide_insert<BITS, 4> : po::k_wide_insert<BITS, 1>;
            auto k_cfill = ww == 16 ? po::k_wide_chain_fill<BITS, 16> : ww == 4 ? po::k_wide_chain_fill<BITS, 4> : po::k_wide_chain_fill<BITS, 1>;
            auto k_fin = ww == 16 ? po::k_wide_finalize<BITS, 16> : ww == 4 ? po::k_wide_finalize<BITS, 4> : po::k_wide_finalize<BITS, 1>;
            hipLaunchKernelGGL(k_ins, dim3(cdiv(n_entries, 256)), dim3(256), 0, st, words, woff, len, n, m,
                               table, tbits, slot_cnt, read_slot, entry_off, slice_build ? a.build_n : 1u, a.build_slice);
            PO_TRY(prefix<uint32_t>(slot_cnt, nslots, slot_start, &h->pinned[0]));
            if (slice_build) {
                // a sub-table's chain segment was sized for its expected share: learn the real number before anything is
                // written (repetitive reads put all their entries into one sub-table)
                HIP_TRY(h, hipStreamSynchronize(st));
                PO_TRY(ws(h->d_chain, (size_t)h->pinned[0] * chain_elem));
                PO_TRY(ws(h->d_chain_tmp, (size_t)h->pinned[0] * chain_elem));
            }
            uint64_t* chain64 = h->d_chain.as<uint64_t>();
            hipLaunchKernelGGL(k_cfill, dim3(cdiv(n_entries, 256)), dim3(256), 0, st, read_slot, entry_off,
                               (uint64_t)n_entries, slot_start, slot_cur, chain64, len);
            sort_chains<uint64_t>();
            hipLaunchKernelGGL(k_fin, dim3(cdiv(nslots, 256)), dim3(256), 0, st, table, nslots, slot_cnt,
                               slot_start, chain64, len);
        }
        // Which reads repeat their own prefix K-mer (selfrep: only their A candidates can be non-longest duplicates)?
        // The narrow whole-set scan finds that as a side effect.  The other cases (own_lists) do not scan every read for it
        // -- a pass over all positions cost 2.2 ms at config 3 with the wide index, and more than the shard's own scan at 8
        // shards -- and settle duplicates inside each read's own candidate list instead (k_select_local).
        HIP_TRY(h, hipGetLastError());
        if (phase_events) HIP_TRY(h, hipEventRecord(h->ev[EV_INDEX], st));
        if (slice_build) {
            // the sub-table and its chain segment are complete in the workspaces: po_index_slice_export copies them out
            HIP_TRY(h, hipStreamSynchronize(st));
            h->sl_tbits = tbits;
            h->sl_entries = h->pinned[0];   // (the prefix sum's total = chain entries of this sub-table)
            if (phase_events) (void)hipEventElapsedTime(&S.ms_index, h->ev[EV_START], h->ev[EV_INDEX]);
            return PO_OK;
        }
        // (a.idx_only, streamed step: the index is built from the first words of every read while piece 0 is still on the
        // wire; the pieces find it valid -- same upload, min_length, flavour -- and reuse it)
        h->idx_valid = a.idx_only || !ext_idx;
        h->idx_gen = h->upload_gen;
        h->idx_m = m;
        h->idx_wide = wide;
        h->idx_tbits = tbits;
        h->idx_bits = (uint32_t)BITS;
        h->idx_ww = ww;
        *done = a.idx_only;
        return PO_OK;
    }

    // ---- scan, counting pass
    po_status scan_count() {
        A.words = words;
        A.tiles = h->d_tiles.as<po::TileRec>();
        A.tile_begin = tile_begin;
        A.tile_end = tile_end;
        A.m = m;
        A.kmask = kmask;
        A.bloom = bloom;
        A.bloom_log2 = bloom_log2;
        A.table = table;
        A.tbits = tbits;
        A.chain = chain;
        A.len = len;
        A.paired = paired;
        A.selfrep = selfrep;
        A.n_selfrep = reinterpret_cast<uint32_t*>(scalars + 2);  // scalars[2] lo: reads with a self-repeating prefix
        A.tile_count = h->d_tile_count.as<uint32_t>();
        A.tile_off = tile_off_p;
        A.truemask = h->d_truemask.as<uint32_t>();
#ifdef PO_STAMPS
        PO_TRY(ws(h->d_flag, (size_t)4096 * 64));
        HIP_TRY(h, hipMemsetAsync(h->d_flag.p, 0, (size_t)4096 * 64, st));
        A.dbg = h->d_flag.as<unsigned long long>();
#endif
        WA.words = words;
        WA.tiles = A.tiles;
        WA.tile_begin = tile_begin;
        WA.tile_end = tile_end;
        WA.m = m;
        WA.table = table;
        WA.tbits = tbits;
        WA.chain = h->d_chain.as<uint64_t>();
        WA.n_slices = 1;
        if (ext_idx) {   // the gathered sliced index: N chunks of [sub-table | chain segment]
            WA.table = static_cast<const po::Slot*>(a.ext_index);
            WA.chain = nullptr;
            WA.n_slices = a.ext_slices;
            WA.chunk_slots = a.ext_chunk_slots;
            WA.chain_off_slots = a.ext_chain_off;
        }
        WA.len = len;
        WA.paired = paired;
        WA.tile_count = A.tile_count;
        WA.lane_slot = A.truemask;
        WA.tile_off = A.tile_off;
        if (wide) {
            if (pair_events) HIP_TRY(h, hipEventRecord(h->ev[EV_PROBE0], st));
            auto wscan = a.streamed ? (ww == 4 ? po::k_wide_scan<BITS, false, BITS == 2, 4> : po::k_wide_scan<BITS, false, BITS == 2, 1>)
                         : ww == 16 ? po::k_wide_scan<BITS, false, false, 16> : ww == 4 ? po::k_wide_scan<BITS, false, false, 4> : po::k_wide_scan<BITS, false, false, 1>;
            hipLaunchKernelGGL(wscan, dim3(cdiv(ntiles, 4)), dim3(256), 0, st, WA, po::CandGuard{nullptr, 0u});
            if (pair_events) HIP_TRY(h, hipEventRecord(h->ev[EV_PROBE1], st));
        } else {
            const size_t scan_lds = (size_t)scan_waves * po::SCAN_LDS_PER_WAVE + bloom_bytes;
            if (scan_lds > h->lds_max) return fail(h, PO_ERR_HIP, "device LDS too small for the scan kernel");
            // (a streamed step -- 2-bit reads only -- has its own instantiations: the reversed pair order is a compile-time choice)
            constexpr bool CAN_STREAM = BITS == 2;
            auto probe_full = a.streamed ? po::k_scan_probe<BITS, true, CAN_STREAM> : po::k_scan_probe<BITS, true, false>;
            auto probe_part = a.streamed ? po::k_scan_probe<BITS, false, CAN_STREAM> : po::k_scan_probe<BITS, false, false>;
            HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(probe_full), hipFuncAttributeMaxDynamicSharedMemorySize, (int)scan_lds));
            HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(probe_part), hipFuncAttributeMaxDynamicSharedMemorySize, (int)scan_lds));
            const uint32_t n_scan_waves = scan_grid * scan_waves;
            PO_TRY(ws(h->d_left, (size_t)n_scan_waves * po::LEFT_CAP * sizeof(uint2)));
            PO_TRY(ws(h->d_left_cnt, (size_t)n_scan_waves * 4));
            PO_TRY(ws(h->d_tile_extra, ((size_t)h->n_tiles + 1) * 4));
            if (fold_clear && self_clean && h->st_selfclean) {
                // nothing to launch
            } else if (fold_clear) {
                const uint32_t te0 = self_clean ? 0u : tile_begin, ten = self_clean ? h->n_tiles : ntiles;
                // (a self-cleaning step's first piece zeroes both parities' scalars; any other reset only its own block)
                hipLaunchKernelGGL(po::k_call_reset, dim3(cdiv(std::max(std::max(n, 16u), std::max(n_scan_waves, ten)), 256)), dim3(256), 0, st,
                                   selfrep, n, self_clean ? h->d_scalars.as<unsigned long long>() : scalars, self_clean ? 16u : 8u,
                                   h->d_left_cnt.as<uint32_t>(), n_scan_waves, h->d_tile_extra.as<uint32_t>() + te0, ten);
            } else {
                HIP_TRY(h, hipMemsetAsync(h->d_left_cnt.p, 0, (size_t)n_scan_waves * 4, st));
                HIP_TRY(h, hipMemsetAsync(h->d_tile_extra.as<uint32_t>() + tile_begin, 0, (size_t)ntiles * 4, st));
            }
            A.left = h->d_left.as<uint2>();
            A.left_cnt = h->d_left_cnt.as<uint32_t>();
            A.tile_extra = h->d_tile_extra.as<uint32_t>();
            if (pair_events) HIP_TRY(h, hipEventRecord(h->ev[EV_PROBE0], st));
            hipLaunchKernelGGL(K == W ? probe_full : probe_part, dim3(scan_grid), dim3(scan_waves * 64), scan_lds, st, A);
            if (pair_events) HIP_TRY(h, hipEventRecord(h->ev[EV_PROBE1], st));
            auto fixup = a.streamed ? po::k_scan_fixup<BITS, CAN_STREAM> : po::k_scan_fixup<BITS, false>;
            hipLaunchKernelGGL(fixup, dim3(n_scan_waves), dim3(256), 0, st, A, n_scan_waves, self_clean ? 1u : 0u);
            // (the leftover counts, tile_extra, are added to the tile counts by the prefix sum of candidate_count)
            if (sw.debug_left) {
                PO_TRY(ensure_host(h, h->scratch_host, (size_t)n_scan_waves * 4));
                HIP_TRY(h, hipMemcpyAsync(h->scratch_host.p, h->d_left_cnt.p, (size_t)n_scan_waves * 4, hipMemcpyDeviceToHost, st));
                HIP_TRY(h, hipStreamSynchronize(st));
                const uint32_t* lc = static_cast<const uint32_t*>(h->scratch_host.p);
                uint64_t sum = 0;
                uint32_t mx = 0;
                for (uint32_t k = 0; k < n_scan_waves; ++k) sum += lc[k], mx = std::max(mx, lc[k]);
                std::fprintf(stderr, "[left] %u scan waves deferred %llu positions (max %u per wave, cap %d)\n", n_scan_waves,
                             (unsigned long long)sum, mx, (int)po::LEFT_CAP);
            }
        }
        HIP_TRY(h, hipGetLastError());
#ifdef PO_STAMPS
        if (!wide) {
            std::vector<unsigned long long> dbg(4096 * 8);
            HIP_TRY(h, hipMemcpyAsync(dbg.data(), h->d_flag.p, dbg.size() * 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(h, hipStreamSynchronize(st));
            double sum[6] = {0, 0, 0, 0, 0, 0};
            for (size_t w = 0; w < 4096; ++w) for (int k = 0; k < 6; ++k) sum[k] += (double)dbg[w * 8 + k];
            if (sum[5] > 0)
                std::fprintf(stderr, "[stamps] per pass (cycles): wait_rw %.0f  filter %.0f  wait_probe %.0f  consume %.0f  issue %.0f  (passes %.0f)\n",
                             sum[0] / sum[5], sum[1] / sum[5], sum[2] / sum[5], sum[3] / sum[5], sum[4] / sum[5], sum[5]);
        }
#endif
        return PO_OK;
    }

    // ---- the candidate count: tile offsets by prefix sum, then the number itself -- waited for, or PREDICTED.
    // A piece of a streamed step whose candidate count is predicted (the same piece of the previous call): nothing
    // waits for the counting pass -- the kernels behind it are launched at once, sized for `cap_c` candidates, and read
    // the real count on the device (CandGuard); the host learns it with the piece's other numbers when it collects the
    // piece.  Needs every per-piece buffer to hold cap_c already (a re-allocation would synchronise the device).
    po_status candidate_count() {
        if (a.streamed && h->st_harvest && h->st_pred_valid && !a.dp && !a.want_cands && !sw.sync_count && !sw.tail_classic) {
            uint64_t pred = h->st_pred_cand[a.shard];
            uint64_t cap = pred + pred / 50 + 256;
            if (sw.pred_scale) cap = pred = (uint64_t)((double)pred * atof(sw.pred_scale));
            const uint64_t worst = cap * 4u;
            bool order = pred >= 400000 && (r_end - r_begin) >= 4096;
            if (sw.verify_order) order = atoi(sw.verify_order) != 0;
            pred_order = order;
            auto fits = [](const DevBuf& b, uint64_t bytes) { return b.p && b.cap >= bytes; };
            async_count = pred > 0 && cap < (16u << 20) && cdiv(cap, po::TAIL_TILE) <= po::TAIL_MAX_TILES &&
                          fits(h->d_cand_a, cap * 4) && fits(h->d_cand_p, cap * 4) && fits(h->d_cand_b, cap * 4) && fits(h->d_type, cap) &&
                          fits(h->d_rowcnt, cap) && fits(h->d_row_off, (cap + 1) * 4) &&
                          fits(h->spare_rows, h->home_on ? cap * sizeof(po::Cand) : worst * sizeof(po_row)) &&
                          (!order || (fits(h->d_vlabel, (uint64_t)(r_end - r_begin) * 4) && fits(h->d_vperm, (uint64_t)(r_end - r_begin) * 4) &&
                                      fits(h->d_vrank, (uint64_t)(r_end - r_begin) * 4))) && h->dev_words < 0xFFFFFFF0ull;
            cap_c = (uint32_t)cap;
        }
        volatile uint64_t* count_slot = async_count ? &h->pinned[zone + 8] : &h->pinned[1];
        volatile uint64_t* also_slot = async_count ? &h->pinned[zone + 9] : &h->pinned[8];
        if (ntiles <= po::PS_SMALL_MAX) {
            PO_TRY(prefix_sum_small(h, A.tile_count + tile_begin, wide ? nullptr : A.tile_extra + tile_begin, ntiles,
                                    tile_off_p + tile_begin, count_slot,
                                    reinterpret_cast<const uint64_t*>(scalars + 2), also_slot, st, reinterpret_cast<uint64_t*>(scalars)));
        } else {
            PO_TRY(prefix_sum<uint32_t>(h, A.tile_count + tile_begin, ntiles, tile_off_p + tile_begin, count_slot,
                                        reinterpret_cast<const uint64_t*>(scalars + 2), also_slot,
                                        wide ? nullptr : A.tile_extra + tile_begin, st, reinterpret_cast<uint64_t*>(scalars), a));
        }
        if (phase_events) HIP_TRY(h, hipEventRecord(h->ev[EV_COUNT], st));
        if (async_count) {
            // (sizes and grids below are for cap_c candidates; the kernels read the real number from scalars[0])
            n_cand64 = cap_c;
            n_selfrep_reads = 0;
            S.n_predicted = 1;
            G.n_dev = scalars;
            G.cap = cap_c;
        } else {
            if (h->st_pend.valid && h->st_harvest) {
                // the previous piece of a streamed step returned with its kernels queued; this piece's counting pass is queued
                // behind them now.  Wait for the previous piece alone, send its rows home, THEN wait for this piece's count:
                // the device is never idle while the host does that, and the rows leave the moment they exist
                HIP_TRY(h, hipEventSynchronize(h->st_pend.ev[EV_DONE]));
                PO_TRY(h->st_harvest());
            }
            HIP_TRY(h, hipStreamSynchronize(st));
            n_cand64 = h->pinned[1];
            n_selfrep_reads = (uint32_t)h->pinned[8];
        }
        if (own_lists || dpE) n_selfrep_reads |= 1u;  // k_select_local may hand repetitive reads to the global selection
        S.n_candidates = n_cand64;
        if (n_cand64 >= 0xFFFFFF00ull)
            return fail(h, PO_ERR_CAPACITY, "candidate count " + std::to_string(n_cand64) + " exceeds one call's capacity (2^32)");
        n_cand = (uint32_t)n_cand64;
        worst_rows = (uint64_t)n_cand * (paired ? 4u : 2u);
        return PO_OK;
    }

    // ---- scan, fill pass; containment candidates whose b has not arrived go onto the deferred list
    po_status scan_fill() {
        PO_TRY(ws_piece(h->d_cand_a, (size_t)n_cand * 4));
        PO_TRY(ws_piece(h->d_cand_p, (size_t)n_cand * 4));
        PO_TRY(ws_piece(h->d_cand_b, (size_t)n_cand * 4));
        PO_TRY(ws_piece(h->d_type, (size_t)n_cand));
        PO_TRY(ws_piece(h->d_rowcnt, (size_t)n_cand));
        PO_TRY(ws_piece(h->d_row_off, ((size_t)n_cand + 1) * 4));
        A.cand_a = h->d_cand_a.as<uint32_t>();
        A.cand_p = h->d_cand_p.as<uint32_t>();
        A.cand_b = h->d_cand_b.as<uint32_t>();
        if (wide) {
            WA.cand_a = A.cand_a;
            WA.cand_p = A.cand_p;
            WA.cand_b = A.cand_b;
            auto wfill = a.streamed ? (ww == 4 ? po::k_wide_scan<BITS, true, BITS == 2, 4> : po::k_wide_scan<BITS, true, BITS == 2, 1>)
                         : ww == 16 ? po::k_wide_scan<BITS, true, false, 16> : ww == 4 ? po::k_wide_scan<BITS, true, false, 4> : po::k_wide_scan<BITS, true, false, 1>;
            hipLaunchKernelGGL(wfill, dim3(cdiv(ntiles, 4)), dim3(256), 0, st, WA, G);
        } else {
            auto fill = a.streamed ? po::k_scan_fill<BITS, BITS == 2> : po::k_scan_fill<BITS, false>;
            hipLaunchKernelGGL(fill, dim3(cdiv(ntiles, 4 * po::FILL_TILES)), dim3(256), 0, st, A, G);
        }
        // locality order of the a-side reads (k_read_label): worth its ~50 us only when the verify is long
        use_order = n_cand >= 400000 && (r_end - r_begin) >= 4096;
        if (sw.verify_order) use_order = atoi(sw.verify_order) != 0;
        if (async_count) use_order = pred_order;   // (decided from the predicted count, before anything was launched)
        use_order = use_order && !a.dp;
        defer_needed = a.streamed && r_end < n;
        if (defer_needed && !use_order) {
            // containment candidates whose b has not arrived: onto the deferred list (the verify kernel skips them);
            // when the locality order is computed, k_read_label's walk over the candidates does this on the way
            hipLaunchKernelGGL(po::k_defer_split, dim3(cdiv(n_cand, 256)), dim3(256), 0, st, A.cand_a, A.cand_p, A.cand_b, n_cand,
                               r_end, h->d_defer.as<po::Cand>(), h->st_defer_cap, h->d_defer.as<uint32_t>() + (size_t)h->st_defer_cap * 4, G);
        }
        HIP_TRY(h, hipGetLastError());
        if (phase_events) HIP_TRY(h, hipEventRecord(h->ev[EV_FILL], st));
        return PO_OK;
    }

    // ---- verify, po_overlaps_ex: banded seed-extension DP, one wave per candidate (extend.hip.h); max_diff = 0 gives the
    // packed compare's answer
    po_status verify_dp() {
        if (2ull * h->max_len + 64ull >= (1ull << 30))   // (the kernel's "infinity" plus the longest sweep must fit 32 bits)
            return fail(h, PO_ERR_CAPACITY, "po_overlaps_ex: reads of 2^29 bases or more are beyond the DP kernel");
        PO_TRY(ws(h->d_end_a, (size_t)n_cand * 4));
        PO_TRY(ws(h->d_end_b, (size_t)n_cand * 4));
        PO_TRY(ws(h->d_dpcnt, 64));
        HIP_TRY(h, hipMemsetAsync(h->d_dpcnt.p, 0, 64, st));
        po::ExtArgs X = {};
        X.words = words;
        X.woff = woff;
        X.len = len;
        X.cand_a = A.cand_a;
        X.cand_p = A.cand_p;
        X.cand_b = A.cand_b;
        X.n_cand = n_cand;
        X.max_diff = dpE;
        X.band = dpW;
        X.paired = paired;
        X.exc_off = h->n_exc_uploaded ? h->d_exc_off.as<uint32_t>() : nullptr;
        X.exc_pos = h->d_exc_pos.as<uint32_t>();
        X.exc_byte = h->d_exc_byte.as<uint8_t>();
        X.type = h->d_type.as<uint8_t>();
        X.end_a = h->d_end_a.as<uint32_t>();
        X.end_b = h->d_end_b.as<uint32_t>();
        X.counters = h->d_dpcnt.as<unsigned long long>();
        S.dp_lanes = dp_bitvec ? 2u : dp_lanes ? 1u : 0u;   // (which of the three mappings: plan())
        if (pair_events) HIP_TRY(h, hipEventRecord(h->ev[EV_VER0], st));
        if (dp_lanes) {
            // candidates ordered by the rows they need, so that the 64 lanes of a wave finish together
            const uint32_t* perm = nullptr;
            bool sorted = n_cand >= 4096;
            if (sw.dp_sort) sorted = atoi(sw.dp_sort) != 0;
            if (sorted) {
                const uint32_t max_bins = (uint32_t)((std::min<size_t>(h->lds_max, 160 * 1024) - 1024) / 4);
                const uint32_t max_rows = h->max_len + dpW;
                uint32_t shift = 0;
                while ((max_rows >> shift) + 1 > max_bins) ++shift;
                const uint32_t n_bins = (max_rows >> shift) + 1;
                const size_t sort_lds = ((size_t)n_bins + po::SORT_BLOCK / 64) * 4;
                PO_TRY(ws(h->d_vlabel, (size_t)n_cand * 4));
                PO_TRY(ws(h->d_vrank, (size_t)n_cand * 4));
                PO_TRY(ws(h->d_vperm, (size_t)n_cand * 4));
                hipLaunchKernelGGL(po::k_dp_rows, dim3(cdiv(n_cand, 256)), dim3(256), 0, st, A.cand_a, A.cand_p, A.cand_b, len, n_cand,
                                   dpW, h->d_vlabel.as<uint32_t>());
                if (sort_lds > 48 * 1024)
                    HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(po::k_read_sort),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)sort_lds));
                hipLaunchKernelGGL(po::k_read_sort, dim3(1), dim3(po::SORT_BLOCK), sort_lds, st, h->d_vlabel.as<uint32_t>(), n_cand,
                                   shift, n_bins, h->d_vrank.as<uint32_t>());
                hipLaunchKernelGGL(po::k_read_invert, dim3(cdiv(n_cand, 256)), dim3(256), 0, st, h->d_vrank.as<uint32_t>(), n_cand, 0u,
                                   h->d_vperm.as<uint32_t>());
                perm = h->d_vperm.as<uint32_t>();
            }
            auto kern = dp_bitvec ? po::k_extend_bits : dpW <= 4 ? po::k_extend_lanes<4> : dpW <= 8 ? po::k_extend_lanes<8> : po::k_extend_lanes<15>;
            hipLaunchKernelGGL(kern, dim3(cdiv(n_cand, 256)), dim3(256), 0, st, X, perm);
        } else {
            hipLaunchKernelGGL((po::k_extend_dp<BITS>), dim3(cdiv(n_cand, 256 / po::WAVE)), dim3(256), 0, st, X);
        }
        if (pair_events) HIP_TRY(h, hipEventRecord(h->ev[EV_VER1], st));
        HIP_TRY(h, hipMemcpyAsync(h->pinned + 32, h->d_dpcnt.p, 16, hipMemcpyDeviceToHost, st));
        return PO_OK;
    }

    // ---- verify, exact: one workgroup per a-side read
    po_status verify_exact() {
        // a's words live in LDS (read length + 3 guard words); reads too long for 64 KB use the global path
        const uint64_t need_words = ((uint64_t)h->max_len + W - 1) / W + 3;
        const uint32_t lds_words_raw = (uint32_t)std::min<uint64_t>(need_words, 8192 - 1100);  // (room for the records in 64 KB)
        const uint32_t n_a = r_end - r_begin;
        const uint32_t* perm = nullptr;
        // (sharded calls too: 0.65 -> 0.51 ms at 2 shards, 0.19 -> 0.17 at 8 -- once the label of a read ranked by
        // the scrambled order was turned back into a read index, see k_read_label)
        if (use_order) {
            // bins of label >> shift, as many as fit into one workgroup's LDS.  Labels are read indices
            // (whole-set calls) or 32-bit scrambled ranks (sharded calls)
            const uint32_t max_bins = (uint32_t)((std::min<size_t>(h->lds_max, 160 * 1024) - 1024) / 4);
            uint32_t shift = 0, n_bins;
            while ((n >> shift) + 1 > max_bins) ++shift;   // labels are read indices in both pairing modes
            n_bins = (n >> shift) + 1;
            const size_t sort_lds = ((size_t)n_bins + po::SORT_BLOCK / 64) * 4;
            PO_TRY(ws(h->d_vlabel, (size_t)n_a * 4));
            PO_TRY(ws(h->d_vperm, (size_t)n_a * 4));
            po::DeferOut dfo = {};
            if (defer_needed) {
                dfo.cand_p = A.cand_p;
                dfo.b_limit = r_end;
                dfo.list = h->d_defer.as<uint4>();
                dfo.cap = h->st_defer_cap;
                dfo.counter = h->d_defer.as<uint32_t>() + (size_t)h->st_defer_cap * 4;
            }
            hipLaunchKernelGGL(po::k_read_label, dim3(cdiv((uint64_t)n_a * 16, 256)), dim3(256), 0, st,
                               h->d_read_tile0.as<uint32_t>(), tile_off_p, A.cand_b, r_begin, n_a, paired,
                               h->d_vlabel.as<uint32_t>(), dfo, G);
            if (sort_lds > 48 * 1024)
                HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(po::k_read_sort),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)sort_lds));
            PO_TRY(ws(h->d_vrank, (size_t)n_a * 4));
            hipLaunchKernelGGL(po::k_read_sort, dim3(1), dim3(po::SORT_BLOCK), sort_lds, st, h->d_vlabel.as<uint32_t>(), n_a,
                               shift, n_bins, h->d_vrank.as<uint32_t>());
            hipLaunchKernelGGL(po::k_read_invert, dim3(cdiv(n_a, 256)), dim3(256), 0, st, h->d_vrank.as<uint32_t>(), n_a, r_begin,
                               h->d_vperm.as<uint32_t>());
            perm = h->d_vperm.as<uint32_t>();
        }
        const uint32_t ver_grid = perm ? 8 * ((n_a + 7) / 8) : n_a;
        auto verify = paired == 2u ? (staged ? po::k_verify_a<BITS, true, true> : po::k_verify_a<BITS, true, false>)
                                   : (staged ? po::k_verify_a<BITS, false, true> : po::k_verify_a<BITS, false, false>);
        if (a.streamed) verify = staged ? po::k_verify_a<BITS, false, true, BITS == 2> : po::k_verify_a<BITS, false, false, BITS == 2>;
        const uint32_t lds_words = (lds_words_raw + 1u) & ~1u;  // even: the records behind a sit on a 16-byte boundary
        const size_t ver_lds = (size_t)lds_words * 8 + (size_t)po::VREC_CAP * sizeof(po::VRec) + 16;
        if (ver_lds > 48 * 1024)
            HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(verify), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ver_lds));
        if (pair_events) HIP_TRY(h, hipEventRecord(h->ev[EV_VER0], st));
        hipLaunchKernelGGL(verify, dim3(ver_grid), dim3(po::VER_BLOCK), ver_lds, st,
                           words, woff, len, h->d_read_tile0.as<uint32_t>(), tile_off_p, A.cand_p,
                           A.cand_b, r_begin, lds_words, paired_ver,
                           h->n_exc_uploaded ? h->d_exc_off.as<uint32_t>() : nullptr, h->d_exc_pos.as<uint32_t>(),
                           h->d_exc_byte.as<uint8_t>(), h->d_type.as<uint8_t>(), perm, n_a, G,
                           sel_in_verify ? selfrep : nullptr, sel_in_verify ? n_deferred : nullptr);
        if (pair_events) HIP_TRY(h, hipEventRecord(h->ev[EV_VER1], st));
        return PO_OK;
    }

    // ---- select inside each read's own list (where the verify kernel has not done it), then which tail
    po_status select_local() {
        ver_timed = true;
        HIP_TRY(h, hipGetLastError());
#ifdef PO_VSTAMPS
        {
            unsigned long long v[64 * 8], z[64 * 8] = {};
            HIP_TRY(h, hipStreamSynchronize(st));
            HIP_TRY(h, hipMemcpyFromSymbol(v, HIP_SYMBOL(po::g_vstamps), sizeof(v)));
            HIP_TRY(h, hipMemcpyToSymbol(HIP_SYMBOL(po::g_vstamps), z, sizeof(z)));
            double sum[8] = {};
            for (int i = 0; i < 64; ++i) for (int k = 0; k < 8; ++k) sum[k] += (double)v[i * 8 + k];
            if (sum[6] > 0)
                std::fprintf(stderr, "[vstamps] per wave (shader clocks): setup %.0f  wait_b %.0f  lds+cmp %.0f  book+init %.0f  life %.0f | iterations %.1f  group-steps/iteration %.2f  waves %.0f\n",
                             sum[0] / sum[6], sum[1] / sum[6], sum[2] / sum[6], sum[3] / sum[6], sum[4] / sum[6], sum[5] / sum[6], sum[7] / sum[5], sum[6]);
        }
#endif
        if (phase_events) HIP_TRY(h, hipEventRecord(h->ev[EV_VERIFY], st));
        if ((own_lists || dpE) && !sel_in_verify) {
            static_assert(po::SEL_CAP == 512, "k_select_local hashes to 9 bits");
            hipLaunchKernelGGL(po::k_select_local, dim3(cdiv(r_end - r_begin, 256 / po::WAVE)), dim3(256), 0, st,
                               h->d_read_tile0.as<uint32_t>(), tile_off_p, A.cand_p, A.cand_b, h->d_type.as<uint8_t>(),
                               r_begin, r_end - r_begin, selfrep, n_deferred, G);
        }
        // A candidate gives at most 2 rows (4 with their mirrors: worst_rows).  When the row buffer kept from an earlier
        // call holds that many, the rows are written without asking the host for their number first.
        // ---- the tail in ONE launch (k_tail: rows per candidate, their prefix sum, the rows, the counters) when the kept
        // row buffer holds the worst case and no global (a, b) table is needed -- or only a gated one: if k_select_local
        // hands a read over after all, k_tail writes nothing but a flag and the classic tail runs instead
        // (rows home in compact form -- h->home_on, po_overlaps_to_host -- : the tail writes one 16-byte record per verified
        // candidate, so its buffer needs n_cand records, not the worst case of rows; a call whose kept buffer is too small
        // makes one here -- never a piece with a predicted count, whose buffers were checked before anything was launched)
        const bool gated_ok = !n_selfrep_reads || (own_lists && n_cand < (16u << 20));
        const bool home_tail_ok = h->home_on && !a.want_cands && !dpE && !sw.tail_classic && gated_ok &&
                                  cdiv(n_cand, po::TAIL_TILE) <= po::TAIL_MAX_TILES;
        if (home_tail_ok && !async_count && h->spare_rows.cap < (size_t)n_cand * sizeof(po::Cand))
            PO_TRY(ws(h->spare_rows, (size_t)n_cand * sizeof(po::Cand) + (a.streamed ? 65536 : 0), false));
        compact_tail = home_tail_ok && h->spare_rows.p && h->spare_rows.cap >= (size_t)n_cand * sizeof(po::Cand);
        can_tail = compact_tail ||
                   (!a.want_cands && !dpE && h->spare_rows.p && h->spare_rows.cap >= worst_rows * sizeof(po_row) && gated_ok &&
                    // (rows left in HBM, whole set: 6.5 M candidates are 0.02 ms faster through the classic kernels)
                    cdiv(n_cand, po::TAIL_TILE) <= (a.streamed || h->home_on ? po::TAIL_MAX_TILES : 4096u) && !sw.tail_classic);
        // (a piece with a predicted count has nothing but the fused tail: the classic kernels take the real count from the host)
        if (async_count && !can_tail) return fail(h, PO_ERR_HIP, "internal: a piece with a predicted candidate count needs the fused tail");
        return PO_OK;
    }

    // ---- the tail in one launch behind k_tile_rows
    po_status fused_tail() {
        const uint32_t n_tt = cdiv(n_cand, po::TAIL_TILE);
        // [tile row sums x n_tt | done counter]; the counter is zero between launches (allocated zero, reset by k_tail)
        if (((size_t)po::TAIL_MAX_TILES + 4) * 4 > h->d_tail_state.cap) {
            PO_TRY(ws(h->d_tail_state, ((size_t)po::TAIL_MAX_TILES + 4) * 4));
            HIP_TRY(h, hipMemsetAsync(h->d_tail_state.p, 0, h->d_tail_state.cap, st));
        }
        uint32_t* tile_rows = h->d_tail_state.as<uint32_t>();
        uint32_t* tail_done = tile_rows + po::TAIL_MAX_TILES;
        const uint32_t* tgate = n_selfrep_reads ? n_deferred : nullptr;
        hipLaunchKernelGGL(compact_tail ? po::k_tile_rows<true> : po::k_tile_rows<false>, dim3(n_tt), dim3(po::TAIL_BLOCK), 0, st, A.cand_a,
                           A.cand_b, h->d_type.as<uint8_t>(), n_cand, paired, tgate, tile_rows, G);
        if (phase_events) HIP_TRY(h, hipEventRecord(h->ev[EV_SELECT], st));
        rows_late = true;
        used_tail = true;
        S.fused_tail = 1;
        res->d_rows = h->spare_rows;
        h->spare_rows = DevBuf();
        tail_zone = async_count ? zone : 48;
        h->pinned[tail_zone] = 0;
        h->pinned[tail_zone + 7] = 0;
        if (compact_tail) {
            res->compact = true;
            hipLaunchKernelGGL(po::k_tail_cands, dim3(n_tt), dim3(po::TAIL_BLOCK), 0, st, A.cand_a, A.cand_p, A.cand_b, h->d_type.as<uint8_t>(),
                               n_cand, res->d_rows.as<po::Cand>(), paired, tgate, tile_rows, n_tt, tail_done,
                               scalars + 3, h->pinned_dev + tail_zone, G, h->home_sh_b, h->home_sh_p);
        } else
        hipLaunchKernelGGL(po::k_tail, dim3(n_tt), dim3(po::TAIL_BLOCK), 0, st, A.cand_a, A.cand_p, A.cand_b, h->d_type.as<uint8_t>(),
                           n_cand, len, res->d_rows.as<po::Row>(), (uint32_t)BITS, paired, tgate, tile_rows, n_tt, tail_done,
                           scalars + 4, h->pinned_dev + tail_zone, G);
        HIP_TRY(h, hipGetLastError());
        return PO_OK;
    }

    // ---- the tail as separate kernels: global selection, row offsets, emit (or the compaction of the multi-GPU form)
    po_status classic_tail() {
        po::PairSlot* ptab = nullptr;
        uint32_t pbits = 0;
        const uint32_t* gate = nullptr;
        uint64_t n_rows64 = 0;
        if (n_selfrep_reads) {
            // some read's prefix recurs inside it (or a read was too repetitive for k_select_local): A candidates
            // of such b may be non-longest duplicates
            uint32_t n_sus;
            if (own_lists && n_cand < (4u << 20)) {
                n_sus = n_cand;  // upper bound: no counting pass, no host round trip (a big call sizes its table exactly)
                gate = n_deferred;  // ... and nothing of it is touched unless k_select_local handed a read over
            } else {
                uint32_t* n_suspect = reinterpret_cast<uint32_t*>(scalars + 2) + 1;
                hipLaunchKernelGGL(po::k_count_suspects, dim3(std::min<uint32_t>(cdiv(n_cand, 256), (uint32_t)h->n_cu * 8)), dim3(256), 0,
                                   st, A.cand_b, h->d_type.as<uint8_t>(), n_cand, selfrep, n_suspect);
                HIP_TRY(h, hipMemcpyAsync(h->pinned + 8, scalars + 2, 8, hipMemcpyDeviceToHost, st));
                HIP_TRY(h, hipStreamSynchronize(st));
                n_sus = (uint32_t)(h->pinned[8] >> 32);
            }
            if (n_sus) {
                pbits = 4;
                while ((1ull << pbits) < 2ull * n_sus) ++pbits;
                PO_TRY(ws_piece(h->d_pair_key, ((size_t)1 << pbits) * sizeof(po::PairSlot)));
                hipLaunchKernelGGL(po::k_fill_gated, dim3((uint32_t)h->n_cu * 8), dim3(256), 0, st, h->d_pair_key.as<uint4>(),
                                   (uint64_t)((size_t)1 << pbits) * sizeof(po::PairSlot) / 16, 0xFFFFFFFFu, gate);
                ptab = h->d_pair_key.as<po::PairSlot>();
                hipLaunchKernelGGL(po::k_select_mark, dim3(cdiv(n_cand, 256)), dim3(256), 0, st, A.cand_a, A.cand_p, A.cand_b,
                                   h->d_type.as<uint8_t>(), n_cand, selfrep, ptab, pbits, gate);
            }
        }
        if (a.want_cands) PO_TRY(ws(h->d_flag, (size_t)n_cand));
        hipLaunchKernelGGL(po::k_select, dim3(cdiv(n_cand, 256)), dim3(256), 0, st, A.cand_a, A.cand_p, A.cand_b,
                           h->d_type.as<uint8_t>(), n_cand, selfrep, ptab, pbits, paired, h->d_rowcnt.as<uint8_t>(),
                           a.want_cands ? h->d_flag.as<uint8_t>() : nullptr, gate);
        HIP_TRY(h, hipGetLastError());
        // A candidate gives at most 2 rows (4 with their mirrors).  When the row buffer kept from an earlier call
        // holds that many, the rows are emitted without asking the host for their number first (one host round
        // trip less per step); the number arrives with the counters at the end.
        if (!a.want_cands) {
            PO_TRY(prefix<uint8_t>(h->d_rowcnt.as<uint8_t>(), n_cand, h->d_row_off.as<uint32_t>(), &h->pinned[2]));
            if (phase_events) HIP_TRY(h, hipEventRecord(h->ev[EV_SELECT], st));
            rows_late = h->spare_rows.p && h->spare_rows.cap >= worst_rows * sizeof(po_row);
            if (!rows_late) {
                HIP_TRY(h, hipStreamSynchronize(st));
                n_rows64 = h->pinned[2];
                if (n_rows64 >= 0xFFFFFF00ull) return fail(h, PO_ERR_CAPACITY, "row count exceeds one call's capacity (2^32)");
            }
            // ---- emit
            PO_TRY(take_row_buffer(h, res, rows_late, n_rows64, worst_rows, a.streamed));
            if (dpE)
                hipLaunchKernelGGL(po::k_emit_ex, dim3(std::min<uint32_t>(cdiv(n_cand, 256), (uint32_t)h->n_cu * 16)), dim3(256), 0,
                                   st, A.cand_a, A.cand_p, A.cand_b, h->d_type.as<uint8_t>(), h->d_end_a.as<uint32_t>(),
                                   h->d_end_b.as<uint32_t>(), h->d_row_off.as<uint32_t>(), n_cand, len,
                                   res->d_rows.as<po::Row>(), (uint32_t)BITS, scalars + 4);
            else
            hipLaunchKernelGGL(po::k_emit, dim3(std::min<uint32_t>(cdiv(n_cand, 256), (uint32_t)h->n_cu * 16)), dim3(256), 0,
                               st, A.cand_a, A.cand_p, A.cand_b, h->d_type.as<uint8_t>(), h->d_row_off.as<uint32_t>(),
                               n_cand, len, res->d_rows.as<po::Row>(), (uint32_t)BITS, paired, scalars + 4);
            HIP_TRY(h, hipGetLastError());
            return PO_OK;
        }
        // ---- multi-GPU form: hand out the verified candidates (one per strand-mirror pair), compacted.  Where the
        // destination is known to be large enough for what the call is expected to keep -- the caller's exchange slot,
        // or a buffer kept from an earlier call that holds even the worst case -- the compaction is queued without
        // asking the host for the number first (one host round trip less per shard call: ~40 us of ~0.5 ms at 8
        // shards); the number arrives with the closing synchronisation, and a slot that turns out too small is
        // handled there (cands_late, finish)
        PO_TRY(prefix<uint8_t>(h->d_flag.as<uint8_t>(), n_cand, h->d_row_off.as<uint32_t>(), &h->pinned[3]));
        if (phase_events) HIP_TRY(h, hipEventRecord(h->ev[EV_SELECT], st));
        po::Cand* dst;
        uint64_t dst_cap;
        if (res->ext_dst && res->ext_cap && !sw.compact_sync) {
            dst = static_cast<po::Cand*>(res->ext_dst);  // straight into the caller's exchange buffer
            dst_cap = res->ext_cap;
            cands_late = true;
            cands_ext = true;
        } else if (h->spare_cands.p && h->spare_cands.cap >= (size_t)n_cand * sizeof(po::Cand) && !sw.compact_sync) {
            res->d_rows = h->spare_cands;
            h->spare_cands = DevBuf();
            dst = res->d_rows.as<po::Cand>();
            dst_cap = n_cand;
            cands_late = true;
        } else {
            HIP_TRY(h, hipStreamSynchronize(st));
            const uint64_t n_ver = h->pinned[3];
            if (res->ext_dst && n_ver <= res->ext_cap) {
                dst = static_cast<po::Cand*>(res->ext_dst);
                res->wrote_ext = true;
            } else {
                if (h->spare_cands.p && h->spare_cands.cap >= n_ver * sizeof(po::Cand)) {
                    res->d_rows = h->spare_cands;
                    h->spare_cands = DevBuf();
                }
                PO_TRY(ws(res->d_rows, std::max<size_t>(n_ver * sizeof(po::Cand), 256), false));
                dst = res->d_rows.as<po::Cand>();
            }
            dst_cap = n_ver;
        }
        cands_cap = dst_cap;
        hipLaunchKernelGGL(po::k_compact, dim3(cdiv(n_cand, 256)), dim3(256), 0, st, A.cand_a, A.cand_p, A.cand_b,
                           h->d_type.as<uint8_t>(), h->d_flag.as<uint8_t>(), h->d_row_off.as<uint32_t>(), n_cand, dst,
                           (uint32_t)std::min<uint64_t>(dst_cap, 0xFFFFFFFFull));
        HIP_TRY(h, hipGetLastError());
        res->elem = sizeof(po::Cand);
        return PO_OK;
    }

    // k_tail found reads handed to the global table: nothing was written -- the classic tail, now
    po_status tail_fallback() {
        h->spare_rows = res->d_rows;
        res->d_rows = DevBuf();
        res->compact = false;
        rows_late = false;
        used_tail = false;
        S.fused_tail = 0;
        S.tail_fallback = 1;
        return classic_tail();
    }

    // (a call without candidates still marks the boundaries of the stages it skipped)
    po_status no_candidates() {
        if (phase_events) HIP_TRY(h, hipEventRecord(h->ev[EV_FILL], st));
        if (phase_events) HIP_TRY(h, hipEventRecord(h->ev[EV_VERIFY], st));
        if (phase_events) HIP_TRY(h, hipEventRecord(h->ev[EV_SELECT], st));
        return PO_OK;
    }

    // ---- the call's end: a piece of a streamed step with its rows in a kept buffer stays pending, any other call waits
    // for its numbers here
    po_status finish() {
        if (pair_events) HIP_TRY(h, hipEventRecord(h->ev[EV_EMIT], st));
        if (!used_tail) HIP_TRY(h, hipMemcpyAsync(h->pinned + 4, scalars + 4, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        res->unique_twins = !a.want_cands && paired != 0 && !dpE;
        HIP_TRY(h, hipEventRecord(h->ev[EV_DONE], st));
        h->st_selfclean = self_clean && used_tail;   // (the next piece of this step may skip its reset)
        if (async_count && h->st_pend.valid) {
            // everything of this piece is queued; now collect the piece before it (its numbers sit in the other zone)
            HIP_TRY(h, hipEventSynchronize(h->st_pend.ev[EV_DONE]));
            PO_TRY(h->st_harvest());
        }
        if (a.streamed && rows_late && h->st_harvest && !h->st_pend.valid) {
            // a piece of a streamed step with its rows in a buffer known to be large enough: nothing here needs the host
            // to wait -- the counts are read when the next piece waits for ITS candidate count (finish_piece)
            po_handle::Pending& P = h->st_pend;
            P.tail = used_tail;
            P.compact = res->compact;
            P.zone = tail_zone;
            P.cap_c = async_count ? cap_c : 0u;
            P.valid = true;
            P.k = a.shard;
            P.S = S;
            P.ver_timed = ver_timed;
            P.full_events = phase_events;
            P.pair_events = pair_events;
            P.ev = h->ev;
            res->count = 0;
            return PO_OK;
        }
        HIP_TRY(h, hipStreamSynchronize(st));
        if (async_count) return fail(h, PO_ERR_HIP, "internal: a piece with a predicted count must stay pending");
        if (used_tail && h->pinned[tail_zone + 7]) {
            PO_TRY(tail_fallback());
            HIP_TRY(h, hipEventRecord(h->ev[EV_EMIT], st));
            HIP_TRY(h, hipMemcpyAsync(h->pinned + 4, scalars + 4, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(h, hipEventRecord(h->ev[EV_DONE], st));
            HIP_TRY(h, hipStreamSynchronize(st));
        }
        if (cands_late) {
            const uint64_t n_ver = h->pinned[3];
            if (n_ver > cands_cap) {
                // the exchange slot was too small for this shard (the caller sizes it from the previous step): once more, into
                // a buffer of the library's own -- the candidate arrays, flags and offsets are all still in place
                PO_TRY(ws(res->d_rows, std::max<size_t>(n_ver * sizeof(po::Cand), 256), false));
                hipLaunchKernelGGL(po::k_compact, dim3(cdiv(n_cand, 256)), dim3(256), 0, st, A.cand_a, A.cand_p, A.cand_b,
                                   h->d_type.as<uint8_t>(), h->d_flag.as<uint8_t>(), h->d_row_off.as<uint32_t>(), n_cand,
                                   res->d_rows.as<po::Cand>(), (uint32_t)n_ver);
                HIP_TRY(h, hipGetLastError());
                HIP_TRY(h, hipStreamSynchronize(st));
            } else if (cands_ext) {
                res->wrote_ext = true;
            }
        }
        // (the fused tail's numbers sit in its zone; the classic kernels' in slots 2 -- rows --, 3 -- candidates kept -- and 4..7)
        const int rows_at = !n_cand ? -1 : used_tail ? tail_zone : a.want_cands ? 3 : 2;
        res->count = close_stats(h, S, rows_at, used_tail ? tail_zone + 1 : 4, h->ev, ver_timed, phase_events, pair_events);
        if (a.want_cands) {
            S.n_verified = res->count;
            S.n_rows = 0;
        }
        if (a.dp && n_cand64) {
            S.dp_steps = h->pinned[32];
            S.dp_stopped = h->pinned[33];
        }
        return PO_OK;
    }
};

template <int BITS>
po_status run_overlaps(po_handle* h, const OverlapArgs& a, po_result* res) {
    OverlapCall<BITS> c(h, a, res);
    bool done = false;
    PO_TRY(c.plan(&done));
    if (done) return PO_OK;
    PO_TRY(c.workspaces());
    PO_TRY(c.build_index(&done));
    if (done) return PO_OK;
    PO_TRY(c.scan_count());
    PO_TRY(c.candidate_count());
    if (c.n_cand) {
        PO_TRY(c.scan_fill());
        PO_TRY(a.dp ? c.verify_dp() : c.verify_exact());
        PO_TRY(c.select_local());
        PO_TRY(c.can_tail ? c.fused_tail() : c.classic_tail());
    } else {
        PO_TRY(c.no_candidates());
    }
    return c.finish();
}

// rows from a (merged) verified-candidate array that lives on this device
po_status run_expand(po_handle* h, const void* d_cands, uint64_t n, po_result* res) {
    hipStream_t st = h->stream;
    po_stats& S = h->stats;
    res->count = 0;
    if (n == 0) return PO_OK;
    if (n >= 0xFFFFFF00ull) return fail(h, PO_ERR_CAPACITY, "candidate count exceeds one call's capacity (2^32)");
    const uint32_t nc = (uint32_t)n;
    const uint32_t paired = (h->bits == 2 && h->paired) ? 1u : 0u;
    PO_TRY(ensure(h, h->d_scalars, 128));
    PO_TRY(ensure(h, h->d_rowcnt, (size_t)nc));
    PO_TRY(ensure(h, h->d_row_off, ((size_t)nc + 1) * 4));
    unsigned long long* scalars = h->d_scalars.as<unsigned long long>();
    const po::Cand* cands = static_cast<const po::Cand*>(d_cands);
    HIP_TRY(h, hipEventRecord(h->ev[EV_SELECT], st));
    HIP_TRY(h, hipMemsetAsync(h->d_scalars.p, 0, 64, st));
    hipLaunchKernelGGL(po::k_cand_rowcnt, dim3(cdiv(nc, 256)), dim3(256), 0, st, cands, nc, (uint32_t)h->len.size(), paired,
                       h->d_rowcnt.as<uint8_t>(), reinterpret_cast<uint32_t*>(scalars + 3));  // [0] is the prefix-sum total
    HIP_TRY(h, hipGetLastError());
    PO_TRY(prefix_sum<uint8_t>(h, h->d_rowcnt.as<uint8_t>(), nc, h->d_row_off.as<uint32_t>(), &h->pinned[2]));
    HIP_TRY(h, hipMemcpyAsync(h->pinned + 3, scalars + 3, 8, hipMemcpyDeviceToHost, st));
    // (as in po_overlaps: a kept row buffer that holds the worst case -- 4 rows per candidate -- is written without
    // waiting for the count; invalid entries have no rows, so emitting before the check writes nothing for them)
    const uint64_t worst_rows = (uint64_t)nc * (paired ? 4u : 2u);
    const bool rows_late = h->spare_rows.p && h->spare_rows.cap >= worst_rows * sizeof(po_row);
    uint64_t n_rows = 0;
    if (!rows_late) {
        HIP_TRY(h, hipStreamSynchronize(st));
        if ((uint32_t)h->pinned[3] != 0) return fail(h, PO_ERR_INVALID, "po_expand: candidate array holds invalid entries");
        n_rows = h->pinned[2];
        if (n_rows >= 0xFFFFFF00ull) return fail(h, PO_ERR_CAPACITY, "row count exceeds one call's capacity (2^32)");
    }
    PO_TRY(take_row_buffer(h, res, rows_late, n_rows, worst_rows));
    HIP_TRY(h, hipMemsetAsync(h->d_scalars.p, 0, 64, st));
    hipLaunchKernelGGL(po::k_emit_cands, dim3(std::min<uint32_t>(cdiv(nc, 256), (uint32_t)h->n_cu * 16)), dim3(256), 0, st,
                       cands, h->d_rowcnt.as<uint8_t>(), h->d_row_off.as<uint32_t>(), nc, h->d_len.as<uint32_t>(),
                       res->d_rows.as<po::Row>(), (uint32_t)h->bits, paired, scalars + 4);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(h->ev[EV_EMIT], st));
    HIP_TRY(h, hipMemcpyAsync(h->pinned + 4, scalars + 4, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    if (rows_late) {
        if ((uint32_t)h->pinned[3] != 0) return fail(h, PO_ERR_INVALID, "po_expand: candidate array holds invalid entries");
        n_rows = h->pinned[2];
    }
    res->count = n_rows;
    res->unique_twins = paired != 0;
    S.n_rows = n_rows;
    S.sum_overlap_bases = h->pinned[5];
    S.verify_bytes_algo = h->pinned[6];
    S.verify_bytes_exec = h->pinned[7];
    (void)hipEventElapsedTime(&S.ms_emit, h->ev[EV_SELECT], h->ev[EV_EMIT]);
    return PO_OK;
}


// ---- layout stage 1 (po_layout_edges): rows -> contained reads + assembly-graph edges ----------

// ids come in strand pairs: ids[2i] = name + "+", ids[2i+1] = name + "-"  (assembler.py:39-40)
bool ids_are_strand_pairs(po_handle* h) {
    if (h->ids_paired >= 0) return h->ids_paired == 1;
    bool ok = (h->ids.size() % 2) == 0;
    for (size_t i = 0; ok && i < h->ids.size(); i += 2) {
        const std::string &p = h->ids[i], &m = h->ids[i + 1];
        ok = !p.empty() && p.size() == m.size() && p.back() == '+' && m.back() == '-' &&
             std::memcmp(p.data(), m.data(), p.size() - 1) == 0;
    }
    h->ids_paired = ok ? 1 : 0;
    return ok;
}

po_status rows_to_device(po_handle* h, po_result* r) {
    if (r->count == 0 || r->d_rows.p) return PO_OK;
    if (!r->host) return fail(h, PO_ERR_INVALID, "result holds no rows");
    PO_TRY(ensure(h, r->d_rows, r->count * r->elem, 1.0, false));
    HIP_TRY(h, hipMemcpyAsync(r->d_rows.p, r->host, r->count * r->elem, hipMemcpyHostToDevice, h->stream));
    return PO_OK;
}

// the node-order buffer of a new edge result: the one a freed result left behind, if it is large enough
po_status ensure_nrank(po_handle* h, po_result* res, size_t bytes) {
    if (!res->d_nrank.p && h->spare_nrank.p && h->spare_nrank.cap >= bytes) {
        res->d_nrank = h->spare_nrank;
        h->spare_nrank = DevBuf();
    }
    return ensure(h, res->d_nrank, bytes, 1.0, false);
}

// the edge buffer of a new edge result, likewise (never less than the smallest allocation)
po_status take_spare_edges(po_handle* h, po_result* res, size_t bytes) {
    if (h->spare_edges.p && h->spare_edges.cap >= bytes) {
        res->d_rows = h->spare_edges;
        h->spare_edges = DevBuf();
    }
    return ensure(h, res->d_rows, std::max<size_t>(bytes, 256), 1.0, false);
}

// all ones behind the ranks of `n_nodes` nodes: the tail of the smallest allocation names no node
po_status fill_nrank_tail(po_handle* h, po_result* res, size_t n_nodes, size_t nrank_bytes) {
    if (n_nodes * 8 < nrank_bytes)
        HIP_TRY(h, hipMemsetAsync(res->d_nrank.as<char>() + n_nodes * 8, 0xFF, nrank_bytes - n_nodes * 8, h->stream));
    return PO_OK;
}

// every buffer a result may hold on the device (an empty one releases nothing)
void release_device(po_result* r) {
    for (DevBuf* b : {&r->d_rows, &r->d_rank, &r->d_nrank, &r->d_moff, &r->d_member, &r->d_prefix, &r->d_mlen, &r->d_ixtable, &r->d_ixval,
                      &r->d_ixoff, &r->d_ixent, &r->d_ixlen})
        b->release();
    for (DevBuf& b : r->d_pp) b.release();
    for (DevBuf* b : {&r->d_wk_rows[0], &r->d_wk_rows[1], &r->d_wk_rl[0], &r->d_wk_rl[1], &r->d_wk_links, &r->d_wk_tmp}) b->release();
    for (DevBuf& b : r->d_rs_rel) b.release();
    for (DevBuf& b : r->d_rs_step) b.release();
    for (DevBuf* b : {&r->d_rs_prev, &r->d_rs_stable, &r->d_rs_global}) b->release();
    // a walk and its live gather know of each other: whichever goes first tells the other
    if (r->rs_live) {
        r->rs_live->rv_stale = true;
        r->rs_live->rv_walk = nullptr;
        r->rs_live = nullptr;
    }
    if (r->rv_walk && r->rv_walk->rs_live == r) r->rv_walk->rs_live = nullptr;
    r->rv_walk = nullptr;
}

// the grid of a kernel that strides over n items: eight workgroups of 256 per CU at the most
uint32_t stride_grid(const po_handle* h, uint64_t n) {
    return std::max<uint32_t>(1u, std::min<uint32_t>(cdiv(n, 256), (uint32_t)h->n_cu * 8));
}

// the workgroups of k_lg_score at the most (one path each per step): eight of 256 threads per CU
uint32_t large_grid_cap(const po_handle* h) { return (uint32_t)h->n_cu * 8; }

// the events of the layout calls, made by the first of them on a handle
po_status lay_events(po_handle* h) {
    for (hipEvent_t& e : h->ev_lay)
        if (!e) HIP_TRY(h, hipEventCreate(&e));
    return PO_OK;
}

// ---- what the stage-2 calls (po_layout_reduce, _tips, _diamonds, _merge) share --------------------------------------
// A driver opens with stage2_open, works out one keep byte and one flag byte per input edge, and closes with
// stage2_count and stage2_emit; between those two it reads its own counters from the landing zone.

// what a stage has worked out per input edge when it closes: keep byte, flag byte, and room for the kept edges' places
struct EdgeMarks {
    const uint8_t* keep;
    const uint8_t* flags;
    uint32_t* koff;
};

// The open: an empty edge result, the bound on the edges (`limit`: what the stage's 32-bit indices allow), with
// `need_order` the node order the stage walks in, the events, the edges on the device.
po_status stage2_open(po_handle* h, po_result* edges, po_result* res, const char* name, uint64_t limit, bool need_order,
                      uint64_t& n_edges_in) {
    res->count = 0;
    res->elem = sizeof(po_edge);
    res->kind_edges = true;
    if (edges->count >= limit) return fail(h, PO_ERR_CAPACITY, std::string(name) + ": too many edges for one call");
    n_edges_in = (uint32_t)edges->count;
    if (need_order) {
        if (!edges->d_nrank.p) return fail(h, PO_ERR_INVALID, std::string(name) + ": the edge result carries no node order");
        if (edges->count && h->len.empty()) return fail(h, PO_ERR_INVALID, std::string(name) + ": edges on a handle without reads");
    }
    PO_TRY(lay_events(h));
    return rows_to_device(h, edges);
}

// The close, first step: the first `n_cnt` counters to words [16..] of the landing zone, the places of the kept edges,
// the flags on their way to the host; waits for all of it.
po_status stage2_count(po_handle* h, uint32_t n, const unsigned long long* cnt, int n_cnt, const EdgeMarks& m, bool want_flags,
                       uint64_t& n_kept) {
    hipStream_t st = h->stream;
    HIP_TRY(h, hipMemcpyAsync(h->pinned + 16, cnt, (size_t)n_cnt * 8, hipMemcpyDeviceToHost, st));
    PO_TRY(prefix_sum<uint8_t>(h, m.keep, n, m.koff, &h->pinned[2]));
    if (want_flags && n) {
        PO_TRY(ensure_host(h, h->scratch_host, n));
        HIP_TRY(h, hipMemcpyAsync(h->scratch_host.p, m.flags, n, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(h, hipStreamSynchronize(st));
    n_kept = h->pinned[2];
    return PO_OK;
}

// The close, second step: the flags to the caller, the kept edges of `src` (and their ranks, where the input has them)
// into the result's buffers -- the buffer of the previous call's result if it is large enough --, the closing event.
po_status stage2_emit(po_handle* h, po_result* res, uint32_t n, uint64_t n_kept, const po::Edge* src, const uint32_t* src_rank,
                      const EdgeMarks& m, uint8_t* flags_out, hipEvent_t done) {
    hipStream_t st = h->stream;
    if (flags_out && n) std::memcpy(flags_out, h->scratch_host.p, n);
    PO_TRY(take_spare_edges(h, res, n_kept * sizeof(po_edge)));
    if (src_rank) PO_TRY(ensure(h, res->d_rank, std::max<size_t>(n_kept * 4, 256), 1.0, false));
    if (n_kept) {
        hipLaunchKernelGGL(po::k_reduce_emit, dim3(cdiv(n, 256)), dim3(256), 0, st, src, src_rank, n, m.keep, m.koff,
                           res->d_rows.as<po::Edge>(), src_rank ? res->d_rank.as<uint32_t>() : nullptr);
        HIP_TRY(h, hipGetLastError());
    }
    HIP_TRY(h, hipEventRecord(done, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    res->count = n_kept;
    return PO_OK;
}

// The rounds of po_layout_tips and po_layout_diamonds go out in batches (the first of `first_batch` rounds, the later
// ones of TIP_BATCH), one readback per batch: `launch(r, word)` enqueues round r, which counts the candidates it leaves
// unresolved in `word`.  A round launched after the last candidate has resolved finds nothing to do.
template <class Launch>
po_status batched_rounds(po_handle* h, uint32_t n_cand, uint32_t first_batch, const char* name, unsigned long long* rcnt,
                         Launch&& launch, uint64_t& rounds_out) {
    hipStream_t st = h->stream;
    uint32_t round = 0;
    for (uint64_t unresolved = n_cand; unresolved;) {
        const uint32_t batch = round == 0 ? first_batch : (uint32_t)TIP_BATCH;
        HIP_TRY(h, hipMemsetAsync(rcnt, 0, (size_t)batch * 8, st));
        for (uint32_t j = 0; j < batch; ++j) launch(round + j, rcnt + j);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(h->pinned + 32, rcnt, (size_t)batch * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipStreamSynchronize(st));
        for (uint32_t j = 0; j < batch && unresolved; ++j, ++round) {
            // (the unresolved candidate of the lowest rank holds its own key everywhere: a round that resolves none is a bug)
            if (h->pinned[32 + j] >= unresolved)
                return fail(h, PO_ERR_HIP, std::string("internal: a round of ") + name + " resolved no candidate");
            unresolved = h->pinned[32 + j];
        }
    }
    rounds_out = round;
    return PO_OK;
}

po_status run_layout(po_handle* h, po_result* rows, const po_layout_params& prm, uint8_t* removed_out, po_result* res) {
    PO_TRY(init_device(h));
    hipStream_t st = h->stream;
    po_layout_stats& L = h->lstats;
    L = po_layout_stats();
    res->count = 0;
    res->elem = sizeof(po_edge);
    res->kind_edges = true;
    const uint32_t n_nodes = (uint32_t)h->len.size();
    const uint64_t n_rows64 = rows->count;
    if (n_rows64 >= 0x7FFFFFF0ull) return fail(h, PO_ERR_CAPACITY, "po_layout_edges: more than 2^31 rows in one call");
    const uint32_t n_rows = (uint32_t)n_rows64;
    const uint32_t n_names = n_nodes / 2;
    L.n_rows = n_rows;
    PO_TRY(lay_events(h));
    hipEvent_t *ev = h->ev_lay + EV_EDGES, *ev_no = h->ev_lay + EV_NODE_ORDER;
    PO_TRY(rows_to_device(h, rows));
    PO_TRY(ensure(h, h->d_lay_len, ((size_t)n_nodes + 1) * 4));
    PO_TRY(ensure(h, h->d_lay_cnt, 128));
    PO_TRY(ensure(h, h->d_scalars, 128));
    PO_TRY(ensure(h, h->d_rflag, (size_t)n_rows + 1));
    PO_TRY(ensure(h, h->d_removed, (size_t)n_names + 1));
    if (n_nodes) HIP_TRY(h, hipMemcpyAsync(h->d_lay_len.p, h->len.data(), (size_t)n_nodes * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemsetAsync(h->d_lay_cnt.p, 0, 128, st));
    HIP_TRY(h, hipMemsetAsync(h->d_removed.p, 0, (size_t)n_names + 1, st));
    unsigned long long* cnt = h->d_lay_cnt.as<unsigned long long>();
    const po::Row* d_rows = rows->d_rows.as<po::Row>();
    const uint32_t* d_len = h->d_lay_len.as<uint32_t>();
    po::LayoutParams P;
    P.min_read_length = prm.min_read_length;
    P.min_overlap_length = prm.min_overlap_length;
    P.max_overhang_abs = prm.max_overhang_abs;
    P.pad = 0;
    P.max_overhang_rel = prm.max_overhang_rel;
    const uint32_t row_grid = stride_grid(h, n_rows);
    HIP_TRY(h, hipEventRecord(ev[0], st));
    if (n_rows) {
        hipLaunchKernelGGL(po::k_layout_classify, dim3(row_grid), dim3(256), 0, st, d_rows, n_rows, d_len, n_nodes, P,
                           h->d_rflag.as<uint8_t>(), h->d_removed.as<uint8_t>(), cnt);
        hipLaunchKernelGGL(po::k_count_bytes, dim3(std::max<uint32_t>(1u, std::min<uint32_t>(cdiv(n_names, 256), 256u))), dim3(256), 0,
                           st, h->d_removed.as<uint8_t>(), n_names, cnt + po::LC_N);
        HIP_TRY(h, hipGetLastError());
    }
    HIP_TRY(h, hipEventRecord(ev[1], st));
    HIP_TRY(h, hipMemcpyAsync(h->pinned + 16, cnt, (po::LC_N + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    const uint64_t* c = h->pinned + 16;
    if (c[po::LC_INVALID]) return fail(h, PO_ERR_INVALID, "po_layout_edges: a row names a read the handle does not hold");
    for (int t = 0; t < 4; ++t) L.n_type[t] = c[po::LC_TYPE0 + t];
    L.n_short = c[po::LC_SHORT];
    L.n_min_overlap = c[po::LC_MINOVL];
    L.n_overhang = c[po::LC_OVERHANG];
    L.n_pass = c[po::LC_PASS];
    L.n_contained_reads = c[po::LC_N];
    uint64_t n_edges = 0;
    if (L.n_pass && rows->unique_twins && !getenv("PHASM_LAYOUT_TABLE")) {
        // rows straight from the paired-strand emission: the last row of an adjacent (row, mirror) group owns the pair
        PO_TRY(ensure(h, h->d_ecnt, (size_t)n_rows));
        PO_TRY(ensure(h, h->d_ewin, (size_t)n_rows));
        PO_TRY(ensure(h, h->d_eoff, ((size_t)n_rows + 1) * 4));
        hipLaunchKernelGGL(po::k_layout_winner_adjacent, dim3(cdiv(n_rows, 256)), dim3(256), 0, st, d_rows, n_rows, d_len,
                           h->d_rflag.as<uint8_t>(), h->d_removed.as<uint8_t>(), h->d_ecnt.as<uint8_t>(), h->d_ewin.as<uint8_t>());
        HIP_TRY(h, hipGetLastError());
        PO_TRY(prefix_sum<uint8_t>(h, h->d_ecnt.as<uint8_t>(), n_rows, h->d_eoff.as<uint32_t>(), &h->pinned[2]));
        HIP_TRY(h, hipEventRecord(ev[2], st));
        HIP_TRY(h, hipStreamSynchronize(st));
        n_edges = h->pinned[2];
        PO_TRY(take_spare_edges(h, res, n_edges * sizeof(po_edge)));
        if (n_edges) {
            hipLaunchKernelGGL(po::k_layout_emit, dim3(cdiv(n_rows, 256)), dim3(256), 0, st, d_rows, n_rows, d_len,
                               h->d_rflag.as<uint8_t>(), h->d_ewin.as<uint8_t>(), h->d_eoff.as<uint32_t>(),
                               res->d_rows.as<po::Edge>(), (const uint32_t*)nullptr, (uint32_t*)nullptr);
            HIP_TRY(h, hipGetLastError());
        }
    } else if (L.n_pass) {
        // twin pair -> last writer row: 2 slots per surviving row (load <= 1/2; 1/4 when every row has its
        // strand-mirror twin), 16-byte slots
        if (2 * L.n_pass + 64 >= 0xFFFFFF00ull) return fail(h, PO_ERR_CAPACITY, "po_layout_edges: too many edges for one call");
        const uint32_t n_slots = (uint32_t)(2 * L.n_pass + 64);
        PO_TRY(ensure(h, h->d_ekey, (size_t)n_slots * sizeof(po::EdgeSlot)));
        PO_TRY(ensure(h, h->d_ecnt, (size_t)n_rows));
        PO_TRY(ensure(h, h->d_ewin, (size_t)n_rows));
        PO_TRY(ensure(h, h->d_eoff, ((size_t)n_rows + 1) * 4));
        PO_TRY(ensure(h, h->d_efirst, (size_t)n_rows * 4));
        HIP_TRY(h, hipMemsetAsync(h->d_ekey.p, 0xFF, (size_t)n_slots * sizeof(po::EdgeSlot), st));
        hipLaunchKernelGGL(po::k_layout_insert, dim3(row_grid), dim3(256), 0, st, d_rows, n_rows, d_len, h->d_rflag.as<uint8_t>(),
                           h->d_removed.as<uint8_t>(), h->d_ekey.as<po::EdgeSlot>(), n_slots);
        hipLaunchKernelGGL(po::k_layout_winner, dim3(cdiv(n_rows, 256)), dim3(256), 0, st, d_rows, n_rows, d_len,
                           h->d_rflag.as<uint8_t>(), h->d_removed.as<uint8_t>(), h->d_ekey.as<po::EdgeSlot>(), n_slots,
                           h->d_ecnt.as<uint8_t>(), h->d_ewin.as<uint8_t>(), h->d_efirst.as<uint32_t>());
        HIP_TRY(h, hipGetLastError());
        PO_TRY(prefix_sum<uint8_t>(h, h->d_ecnt.as<uint8_t>(), n_rows, h->d_eoff.as<uint32_t>(), &h->pinned[2]));
        HIP_TRY(h, hipEventRecord(ev[2], st));
        HIP_TRY(h, hipStreamSynchronize(st));
        n_edges = h->pinned[2];
        PO_TRY(take_spare_edges(h, res, n_edges * sizeof(po_edge)));
        PO_TRY(ensure(h, res->d_rank, std::max<size_t>(n_edges * 4, 256), 1.0, false));
        if (n_edges) {
            hipLaunchKernelGGL(po::k_layout_emit, dim3(cdiv(n_rows, 256)), dim3(256), 0, st, d_rows, n_rows, d_len,
                               h->d_rflag.as<uint8_t>(), h->d_ewin.as<uint8_t>(), h->d_eoff.as<uint32_t>(),
                               res->d_rows.as<po::Edge>(), h->d_efirst.as<uint32_t>(), res->d_rank.as<uint32_t>());
            HIP_TRY(h, hipGetLastError());
        }
    } else {
        HIP_TRY(h, hipEventRecord(ev[2], st));
    }
    HIP_TRY(h, hipEventRecord(ev[3], st));
    // the node order of this graph, for po_layout_tips.  Outside the times above, which are stage 1 as it was; these two
    // passes have times of their own (po_get_node_order_stats)
    po_node_order_stats& NO = h->nostats;
    NO = po_node_order_stats();
    NO.n_rows = n_rows;
    PO_TRY(ensure_nrank(h, res, std::max<size_t>((size_t)n_nodes * 8, 256)));
    HIP_TRY(h, hipEventRecord(ev_no[0], st));
    HIP_TRY(h, hipMemsetAsync(res->d_nrank.p, 0xFF, std::max<size_t>((size_t)n_nodes * 8, 256), st));
    if (L.n_pass) {
        PO_TRY(ensure(h, h->d_lay_firstc, ((size_t)n_nodes + 1) * 4));
        HIP_TRY(h, hipMemsetAsync(h->d_lay_firstc.p, 0xFF, ((size_t)n_nodes + 1) * 4, st));
        hipLaunchKernelGGL(po::k_layout_first_contained, dim3(row_grid), dim3(256), 0, st, d_rows, n_rows,
                           h->d_rflag.as<uint8_t>(), h->d_lay_firstc.as<uint32_t>());
        HIP_TRY(h, hipEventRecord(ev_no[1], st));
        hipLaunchKernelGGL(po::k_layout_node_rank, dim3(row_grid), dim3(256), 0, st, d_rows, n_rows, h->d_rflag.as<uint8_t>(),
                           h->d_removed.as<uint8_t>(), h->d_lay_firstc.as<uint32_t>(), res->d_nrank.as<unsigned long long>());
        HIP_TRY(h, hipGetLastError());
    }
    HIP_TRY(h, hipEventRecord(ev_no[2], st));
    if (removed_out && n_names) {
        PO_TRY(ensure_host(h, h->scratch_host, n_names));
        HIP_TRY(h, hipMemcpyAsync(h->scratch_host.p, h->d_removed.p, n_names, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(h, hipStreamSynchronize(st));
    if (removed_out && n_names) std::memcpy(removed_out, h->scratch_host.p, n_names);
    res->count = n_edges;
    L.n_edges = n_edges;
    (void)hipEventElapsedTime(&L.ms_classify, ev[0], ev[1]);
    (void)hipEventElapsedTime(&L.ms_dedupe, ev[1], ev[2]);
    (void)hipEventElapsedTime(&L.ms_emit, ev[2], ev[3]);
    (void)hipEventElapsedTime(&L.ms_total, ev[0], ev[3]);
    if (L.n_pass) {
        (void)hipEventElapsedTime(&NO.ms_first_contained, ev_no[0], ev_no[1]);
        (void)hipEventElapsedTime(&NO.ms_rank, ev_no[1], ev_no[2]);
    }
    (void)hipEventElapsedTime(&NO.ms_total, ev_no[0], ev_no[2]);
    return PO_OK;
}

// ---- transitive reduction + make_symmetric (po_layout_reduce): edges -> flags + kept edges ------

po_status run_reduce(po_handle* h, po_result* edges, const po_reduce_params& prm, uint8_t* flags_out, po_result* res) {
    hipStream_t st = h->stream;
    po_reduce_stats& R = h->rstats;
    R = po_reduce_stats();
    const uint32_t n_nodes = (uint32_t)h->len.size();
    PO_TRY(stage2_open(h, edges, res, "po_layout_reduce", 0xFFFFFF00ull, false, R.n_edges_in));
    const uint32_t n = (uint32_t)edges->count;
    hipEvent_t* ev = h->ev_lay + EV_REDUCE;
    if (edges->d_nrank.p) {   // the node order goes with the graph: the reduction removes edges, never nodes
        const size_t nb = std::max<size_t>((size_t)n_nodes * 8, 256);
        PO_TRY(ensure_nrank(h, res, nb));
        HIP_TRY(h, hipMemcpyAsync(res->d_nrank.p, edges->d_nrank.p, nb, hipMemcpyDeviceToDevice, st));
    }
    if (n == 0 || n_nodes == 0) {
        if (n) return fail(h, PO_ERR_INVALID, "po_layout_reduce: edges on a handle without reads");
        PO_TRY(ensure(h, res->d_rows, 256, 1.0, false));
        HIP_TRY(h, hipStreamSynchronize(st));
        return PO_OK;
    }
    const size_t nn = (size_t)n_nodes + 1, ne = (size_t)n;
    PO_TRY(ensure(h, h->d_scalars, 128));
    DevBuf* B = h->d_red;
    PO_TRY(ensure(h, B[RB_CNT], 128));
    for (int k : {RB_DEG, RB_OFF, RB_CUR}) PO_TRY(ensure(h, B[k], nn * 4));
    PO_TRY(ensure(h, B[RB_TKEY], ne * 8));
    for (int k : {RB_TTGT, RB_TEID, RB_CTGT, RB_CW, RB_CEID, RB_CIDPOS, RB_STGT, RB_SEID}) PO_TRY(ensure(h, B[k], ne * 4));
    PO_TRY(ensure(h, B[RB_KOFF], (ne + 1) * 4));
    for (int k : {RB_STATE, RB_FLAG1, RB_FLAGS, RB_KEEP}) PO_TRY(ensure(h, B[k], ne));
    const po::Edge* d_edges = edges->d_rows.as<po::Edge>();
    const uint32_t* d_rank = edges->d_rank.p ? edges->d_rank.as<uint32_t>() : nullptr;
    unsigned long long *cnt = B[RB_CNT].as<unsigned long long>(), *tkey = B[RB_TKEY].as<unsigned long long>();
    uint32_t *deg = B[RB_DEG].as<uint32_t>(), *off = B[RB_OFF].as<uint32_t>(), *cur = B[RB_CUR].as<uint32_t>(),
             *ttgt = B[RB_TTGT].as<uint32_t>(), *teid = B[RB_TEID].as<uint32_t>(), *ctgt = B[RB_CTGT].as<uint32_t>(),
             *ceid = B[RB_CEID].as<uint32_t>(), *cidpos = B[RB_CIDPOS].as<uint32_t>(), *stgt = B[RB_STGT].as<uint32_t>(),
             *seid = B[RB_SEID].as<uint32_t>(), *koff = B[RB_KOFF].as<uint32_t>();
    int32_t* cw = B[RB_CW].as<int32_t>();
    uint8_t *state = B[RB_STATE].as<uint8_t>(), *flag1 = B[RB_FLAG1].as<uint8_t>(), *flags = B[RB_FLAGS].as<uint8_t>(),
            *keep = B[RB_KEEP].as<uint8_t>();
    const uint32_t edge_grid = stride_grid(h, n);
    HIP_TRY(h, hipMemsetAsync(cnt, 0, 128, st));
    HIP_TRY(h, hipMemsetAsync(deg, 0, nn * 4, st));
    HIP_TRY(h, hipMemsetAsync(cur, 0, nn * 4, st));
    HIP_TRY(h, hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(po::k_reduce_degree, dim3(edge_grid), dim3(256), 0, st, d_edges, n, n_nodes, deg, cnt);
    hipLaunchKernelGGL(po::k_reduce_maxdeg, dim3(std::max<uint32_t>(1u, std::min<uint32_t>(cdiv(n_nodes, 256), 256u))), dim3(256), 0, st,
                       deg, n_nodes, cnt);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(h->pinned + 16, cnt, po::RC_N * 8, hipMemcpyDeviceToHost, st));
    PO_TRY(prefix_sum<uint32_t>(h, deg, n_nodes, off, &h->pinned[2]));
    HIP_TRY(h, hipStreamSynchronize(st));
    // (an edge that names a node the handle does not hold would index out of the CSR: nothing is scattered then)
    if (h->pinned[16 + po::RC_INVALID]) return fail(h, PO_ERR_INVALID, "po_layout_reduce: an edge names a read the handle does not hold");
    R.max_out_degree = h->pinned[16 + po::RC_MAXDEG];
    hipLaunchKernelGGL(po::k_reduce_scatter, dim3(cdiv(n, 256)), dim3(256), 0, st, d_edges, d_rank, n, off, cur, tkey, ttgt, teid);
    hipLaunchKernelGGL(po::k_reduce_order, dim3(cdiv(n, 256)), dim3(256), 0, st, d_edges, n, off, deg, tkey, ttgt, teid, ctgt, cw, ceid,
                       cidpos, stgt, seid);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(ev[1], st));
    hipLaunchKernelGGL(po::k_reduce_mark, dim3(n_nodes), dim3(po::WAVE), 0, st, n_nodes, prm.length_fuzz, off, deg, ctgt, cw, ceid,
                       cidpos, stgt, state, flag1);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(ev[2], st));
    hipLaunchKernelGGL(po::k_reduce_symmetric, dim3(edge_grid), dim3(256), 0, st, d_edges, n, off, deg, stgt, seid, flag1, flags, keep,
                       cnt);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(ev[3], st));
    uint64_t n_kept = 0;
    const EdgeMarks marks = {keep, flags, koff};
    PO_TRY(stage2_count(h, n, cnt, po::RC_N, marks, flags_out != nullptr, n_kept));
    R.n_transitive = h->pinned[16 + po::RC_TRANSITIVE];
    R.n_asymmetric = h->pinned[16 + po::RC_ASYMMETRIC];
    R.n_edges_out = n_kept;
    PO_TRY(stage2_emit(h, res, n, n_kept, d_edges, d_rank, marks, flags_out, ev[4]));
    (void)hipEventElapsedTime(&R.ms_csr, ev[0], ev[1]);
    (void)hipEventElapsedTime(&R.ms_mark, ev[1], ev[2]);
    (void)hipEventElapsedTime(&R.ms_symmetric, ev[2], ev[3]);
    (void)hipEventElapsedTime(&R.ms_emit, ev[3], ev[4]);
    (void)hipEventElapsedTime(&R.ms_total, ev[0], ev[4]);
    return PO_OK;
}

// ---- tip removal + make_symmetric + clean_graph (po_layout_tips): edges -> flags + kept edges + node order ------

po_status run_tips(po_handle* h, po_result* edges, const po_tips_params& prm, uint8_t* flags_out, po_result* res) {
    hipStream_t st = h->stream;
    po_tips_stats& T = h->tstats;
    T = po_tips_stats();
    const uint32_t n_nodes = (uint32_t)h->len.size();
    PO_TRY(stage2_open(h, edges, res, "po_layout_tips", 0x7FFFFF00ull, true, T.n_edges_in));
    const uint32_t n = (uint32_t)edges->count;
    hipEvent_t* ev = h->ev_lay + EV_TIPS;
    const size_t nn = (size_t)n_nodes + 1, ne = (size_t)n + 1;
    const uint32_t n_slots = 2 * n + 64;
    DevBuf* B = h->d_tip;
    PO_TRY(ensure(h, h->d_scalars, 128));
    PO_TRY(ensure(h, B[TB_CNT], 128));
    PO_TRY(ensure(h, B[TB_RCNT], TIP_BATCH * 8));
    for (int k : {TB_OUTDEG, TB_OUTSUM, TB_INDEG, TB_INSUM, TB_CAND}) PO_TRY(ensure(h, B[k], nn * 4));
    PO_TRY(ensure(h, B[TB_MARK], nn * 8));
    for (int k : {TB_CSTATE, TB_ALIVE}) PO_TRY(ensure(h, B[k], nn));
    for (int k : {TB_EFLAG, TB_FLAGS, TB_KEEP}) PO_TRY(ensure(h, B[k], ne));
    PO_TRY(ensure(h, B[TB_KOFF], (ne + 1) * 4));
    PO_TRY(ensure(h, B[TB_TKEY], (size_t)n_slots * 8));
    PO_TRY(ensure(h, B[TB_TVAL], (size_t)n_slots * 4));
    const size_t nrank_bytes = std::max<size_t>((size_t)n_nodes * 8, 256);
    PO_TRY(ensure_nrank(h, res, nrank_bytes));
    const po::Edge* d_edges = edges->d_rows.as<po::Edge>();
    const uint32_t* d_rank = edges->d_rank.p ? edges->d_rank.as<uint32_t>() : nullptr;
    const unsigned long long* nrank = edges->d_nrank.as<unsigned long long>();
    unsigned long long *cnt = B[TB_CNT].as<unsigned long long>(), *rcnt = B[TB_RCNT].as<unsigned long long>();
    uint32_t *outdeg = B[TB_OUTDEG].as<uint32_t>(), *outsum = B[TB_OUTSUM].as<uint32_t>(), *indeg = B[TB_INDEG].as<uint32_t>(),
             *insum = B[TB_INSUM].as<uint32_t>(), *cand = B[TB_CAND].as<uint32_t>();
    unsigned long long* mark = B[TB_MARK].as<unsigned long long>();
    uint8_t *cstate = B[TB_CSTATE].as<uint8_t>(), *eflag = B[TB_EFLAG].as<uint8_t>(), *flags = B[TB_FLAGS].as<uint8_t>(),
            *keep = B[TB_KEEP].as<uint8_t>(), *alive = B[TB_ALIVE].as<uint8_t>();
    unsigned long long* tkey = B[TB_TKEY].as<unsigned long long>();
    uint32_t *tval = B[TB_TVAL].as<uint32_t>(), *koff = B[TB_KOFF].as<uint32_t>();
    const uint32_t edge_grid = stride_grid(h, n), node_grid = stride_grid(h, n_nodes);
    // No truncation of the caller's bound: a walk never visits a node twice (its start has no in-edge, and every later
    // node has exactly one when the walk leaves it -- tips.hip.h), so it holds at most n_nodes
    // nodes and any bound of n_nodes or more decides as n_nodes does.  The cap keeps `max_len + 2` from wrapping and
    // the chains that k_tips_mark follows, which do not stop at a visited node, short.
    const uint32_t max_len = std::min<uint32_t>(prm.max_tip_len, n_nodes);
    HIP_TRY(h, hipMemsetAsync(cnt, 0, 128, st));
    for (uint32_t* p : {outdeg, outsum, indeg, insum}) HIP_TRY(h, hipMemsetAsync(p, 0, nn * 4, st));
    HIP_TRY(h, hipMemsetAsync(alive, 0, nn, st));
    HIP_TRY(h, hipMemsetAsync(tkey, 0xFF, (size_t)n_slots * 8, st));
    HIP_TRY(h, hipEventRecord(ev[0], st));
    if (n) {
        hipLaunchKernelGGL(po::k_tips_degree, dim3(edge_grid), dim3(256), 0, st, d_edges, n, n_nodes, outdeg, outsum, indeg, insum,
                           eflag, cnt);
        hipLaunchKernelGGL(po::k_tips_insert, dim3(edge_grid), dim3(256), 0, st, d_edges, n, tkey, tval, n_slots);
        HIP_TRY(h, hipGetLastError());
    }
    HIP_TRY(h, hipMemcpyAsync(h->pinned + 16, cnt, po::TC_N * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipEventRecord(ev[1], st));
    HIP_TRY(h, hipStreamSynchronize(st));
    // (an edge that names a node the handle does not hold would index out of the degree arrays: nothing walks then)
    if (h->pinned[16 + po::TC_INVALID]) return fail(h, PO_ERR_INVALID, "po_layout_tips: an edge names a read the handle does not hold");
    // one pass of remove_incoming_tips (rev = 0) or remove_outgoing_tips (rev = 1): rounds until every candidate is resolved
    auto pass = [&](int rev, uint8_t which, uint64_t& n_cand_out, uint64_t& rounds_out) -> po_status {
        po::TipSide g = rev ? po::TipSide{indeg, insum, outdeg, outsum} : po::TipSide{outdeg, outsum, indeg, insum};
        n_cand_out = rounds_out = 0;
        if (n == 0) return PO_OK;
        HIP_TRY(h, hipMemsetAsync(mark, 0xFF, nn * 8, st));
        HIP_TRY(h, hipMemsetAsync(cnt + po::TC_CAND, 0, 8, st));
        hipLaunchKernelGGL(po::k_tips_candidates, dim3(cdiv(n_nodes, 256)), dim3(256), 0, st, n_nodes, nrank, g.fdeg, g.bdeg, cand,
                           cstate, cnt);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(h->pinned + 16, cnt + po::TC_CAND, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipStreamSynchronize(st));
        const uint32_t n_cand = (uint32_t)h->pinned[16];
        n_cand_out = n_cand;
        return batched_rounds(h, n_cand, 8, "po_layout_tips", rcnt, [&](uint32_t r, unsigned long long* left) {
            hipLaunchKernelGGL(po::k_tips_mark, dim3(cdiv(n_cand, 256)), dim3(256), 0, st, d_edges, n, rev, max_len, r, cand, cstate,
                               n_cand, nrank, g.fdeg, g.fsum, mark);
            hipLaunchKernelGGL(po::k_tips_resolve, dim3(cdiv(n_cand, 256)), dim3(256), 0, st, d_edges, n, rev, max_len,
                               prm.max_tip_len_bases, r, which, cand, cstate, n_cand, nrank, g, mark, eflag, left);
        }, rounds_out);
    };
    PO_TRY(pass(0, 1, T.n_candidates_in, T.n_rounds_in));
    HIP_TRY(h, hipEventRecord(ev[2], st));
    PO_TRY(pass(1, 2, T.n_candidates_out, T.n_rounds_out));
    HIP_TRY(h, hipEventRecord(ev[3], st));
    if (n) {
        hipLaunchKernelGGL(po::k_tips_symmetric, dim3(edge_grid), dim3(256), 0, st, d_edges, n, tkey, tval, n_slots, eflag, flags,
                           keep, cnt);
        hipLaunchKernelGGL(po::k_tips_alive, dim3(edge_grid), dim3(256), 0, st, d_edges, n, keep, alive);
    }
    hipLaunchKernelGGL(po::k_tips_nodes, dim3(node_grid), dim3(256), 0, st, n_nodes, nrank, alive,
                       res->d_nrank.as<unsigned long long>(), cnt);
    HIP_TRY(h, hipGetLastError());
    PO_TRY(fill_nrank_tail(h, res, n_nodes, nrank_bytes));
    HIP_TRY(h, hipEventRecord(ev[4], st));
    uint64_t n_kept = 0;
    const EdgeMarks marks = {keep, flags, koff};
    PO_TRY(stage2_count(h, n, cnt, po::TC_N, marks, flags_out != nullptr, n_kept));
    T.n_in_tip_edges = h->pinned[16 + po::TC_IN];
    T.n_out_tip_edges = h->pinned[16 + po::TC_OUT];
    T.n_asymmetric = h->pinned[16 + po::TC_ASYM];
    T.n_nodes = h->pinned[16 + po::TC_NODES];
    T.n_isolated_nodes = h->pinned[16 + po::TC_ISOLATED];
    T.n_edges_out = n_kept;
    PO_TRY(stage2_emit(h, res, n, n_kept, d_edges, d_rank, marks, flags_out, ev[5]));
    (void)hipEventElapsedTime(&T.ms_setup, ev[0], ev[1]);
    (void)hipEventElapsedTime(&T.ms_incoming, ev[1], ev[2]);
    (void)hipEventElapsedTime(&T.ms_outgoing, ev[2], ev[3]);
    (void)hipEventElapsedTime(&T.ms_symmetric, ev[3], ev[4]);
    (void)hipEventElapsedTime(&T.ms_emit, ev[4], ev[5]);
    (void)hipEventElapsedTime(&T.ms_total, ev[0], ev[5]);
    return PO_OK;
}

// ---- remove_diamond_tips (po_layout_diamonds): edges -> flags + kept edges + node order ---------------------------

po_status run_diamonds(po_handle* h, po_result* edges, uint8_t* flags_out, po_result* res) {
    hipStream_t st = h->stream;
    po_diamond_stats& D = h->dstats;
    D = po_diamond_stats();
    const uint32_t n_nodes = (uint32_t)h->len.size();
    PO_TRY(stage2_open(h, edges, res, "po_layout_diamonds", 0x7FFFFF00ull, true, D.n_edges_in));
    const uint32_t n = (uint32_t)edges->count;
    hipEvent_t* ev = h->ev_lay + EV_DIAMONDS;
    // the workspaces of po_layout_tips under other names (grow-only, on the handle): OUTSUM / INSUM hold the min / max id
    // of a node's in-edges, ALIVE the removed byte per node
    const size_t nn = (size_t)n_nodes + 1, ne = (size_t)n + 1;
    DevBuf* B = h->d_tip;
    PO_TRY(ensure(h, h->d_scalars, 128));
    PO_TRY(ensure(h, B[TB_CNT], 128));
    PO_TRY(ensure(h, B[TB_RCNT], TIP_BATCH * 8));
    for (int k : {TB_OUTDEG, TB_OUTSUM, TB_INDEG, TB_INSUM, TB_CAND}) PO_TRY(ensure(h, B[k], nn * 4));
    PO_TRY(ensure(h, B[TB_MARK], nn * 8));
    for (int k : {TB_CSTATE, TB_ALIVE}) PO_TRY(ensure(h, B[k], nn));
    for (int k : {TB_EFLAG, TB_KEEP}) PO_TRY(ensure(h, B[k], ne));
    PO_TRY(ensure(h, B[TB_KOFF], (ne + 1) * 4));
    const size_t nrank_bytes = std::max<size_t>((size_t)n_nodes * 8, 256);
    PO_TRY(ensure_nrank(h, res, nrank_bytes));
    const po::Edge* d_edges = edges->d_rows.as<po::Edge>();
    const uint32_t* d_rank = edges->d_rank.p ? edges->d_rank.as<uint32_t>() : nullptr;
    const unsigned long long* nrank = edges->d_nrank.as<unsigned long long>();
    unsigned long long *cnt = B[TB_CNT].as<unsigned long long>(), *rcnt = B[TB_RCNT].as<unsigned long long>();
    uint32_t *outdeg = B[TB_OUTDEG].as<uint32_t>(), *indeg = B[TB_INDEG].as<uint32_t>(), *inmin = B[TB_OUTSUM].as<uint32_t>(),
             *inmax = B[TB_INSUM].as<uint32_t>(), *cand = B[TB_CAND].as<uint32_t>(), *koff = B[TB_KOFF].as<uint32_t>();
    unsigned long long* mark = B[TB_MARK].as<unsigned long long>();
    uint8_t *cstate = B[TB_CSTATE].as<uint8_t>(), *eflag = B[TB_EFLAG].as<uint8_t>(), *keep = B[TB_KEEP].as<uint8_t>(),
            *removed = B[TB_ALIVE].as<uint8_t>();
    const uint32_t edge_grid = stride_grid(h, n), both_grid = stride_grid(h, std::max(n, n_nodes));
    HIP_TRY(h, hipMemsetAsync(cnt, 0, 128, st));
    for (uint32_t* p : {outdeg, indeg, inmax}) HIP_TRY(h, hipMemsetAsync(p, 0, nn * 4, st));
    HIP_TRY(h, hipMemsetAsync(inmin, 0xFF, nn * 4, st));
    HIP_TRY(h, hipMemsetAsync(mark, 0xFF, nn * 8, st));
    HIP_TRY(h, hipEventRecord(ev[0], st));
    if (n) {
        hipLaunchKernelGGL(po::k_diamond_degree, dim3(edge_grid), dim3(256), 0, st, d_edges, n, n_nodes, outdeg, indeg, inmin, inmax,
                           eflag, cnt);
        HIP_TRY(h, hipGetLastError());
    }
    if (n_nodes) {
        // (in stream order behind the degrees; with an invalid edge the degrees are incomplete and nothing is decided on them)
        hipLaunchKernelGGL(po::k_diamond_candidates, dim3(cdiv(n_nodes, 256)), dim3(256), 0, st, n_nodes, nrank, outdeg, indeg, cand,
                           cstate, removed, cnt);
        HIP_TRY(h, hipGetLastError());
    }
    HIP_TRY(h, hipMemcpyAsync(h->pinned + 16, cnt, po::DC_N * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipEventRecord(ev[1], st));
    HIP_TRY(h, hipStreamSynchronize(st));
    D.n_invalid = h->pinned[16 + po::DC_INVALID];
    // (an edge that names a node the handle does not hold would index out of the degree arrays: nothing is decided then)
    if (D.n_invalid) return fail(h, PO_ERR_INVALID, "po_layout_diamonds: an edge names a read the handle does not hold");
    const uint32_t n_cand = (uint32_t)h->pinned[16 + po::DC_CAND];
    D.n_candidates = n_cand;
    PO_TRY(batched_rounds(h, n_cand, 4, "po_layout_diamonds", rcnt, [&](uint32_t r, unsigned long long* left) {
        hipLaunchKernelGGL(po::k_diamond_mark, dim3(cdiv(n_cand, 256)), dim3(256), 0, st, d_edges, n, r, cand, cstate, n_cand, nrank,
                           indeg, inmin, inmax, mark);
        hipLaunchKernelGGL(po::k_diamond_resolve, dim3(cdiv(n_cand, 256)), dim3(256), 0, st, d_edges, n, r, cand, cstate, n_cand,
                           nrank, outdeg, indeg, inmin, inmax, mark, eflag, removed, left, cnt);
    }, D.n_rounds));
    HIP_TRY(h, hipEventRecord(ev[2], st));
    if (n || n_nodes) {
        hipLaunchKernelGGL(po::k_diamond_nodes, dim3(both_grid), dim3(256), 0, st, n, n_nodes, eflag, keep, nrank, removed,
                           res->d_nrank.as<unsigned long long>(), cnt);
        HIP_TRY(h, hipGetLastError());
    }
    PO_TRY(fill_nrank_tail(h, res, n_nodes, nrank_bytes));
    uint64_t n_kept = 0;
    const EdgeMarks marks = {keep, eflag, koff};
    PO_TRY(stage2_count(h, n, cnt, po::DC_N, marks, flags_out != nullptr, n_kept));
    D.n_diamonds = h->pinned[16 + po::DC_DIAMONDS];
    D.n_nodes = h->pinned[16 + po::DC_NODES];
    D.n_nodes_removed = h->pinned[16 + po::DC_REMOVED];
    D.n_edges_out = n_kept;
    PO_TRY(stage2_emit(h, res, n, n_kept, d_edges, d_rank, marks, flags_out, ev[3]));
    (void)hipEventElapsedTime(&D.ms_setup, ev[0], ev[1]);
    (void)hipEventElapsedTime(&D.ms_rounds, ev[1], ev[2]);
    (void)hipEventElapsedTime(&D.ms_emit, ev[2], ev[3]);
    (void)hipEventElapsedTime(&D.ms_total, ev[0], ev[3]);
    return PO_OK;
}

// ---- merge_unambiguous_paths (po_layout_merge): edges -> flags + renamed kept edges + merged-node tables + node order ----

po_status run_merge(po_handle* h, po_result* edges, uint8_t* flags_out, po_result* res) {
    hipStream_t st = h->stream;
    po_merge_stats& M = h->mstats;
    M = po_merge_stats();
    res->merged = true;
    const uint32_t n_nodes = (uint32_t)h->len.size();
    PO_TRY(stage2_open(h, edges, res, "po_layout_merge", 0x7FFFFF00ull, true, M.n_edges_in));
    const uint32_t n = (uint32_t)edges->count;
    hipEvent_t* ev = h->ev_lay + EV_MERGE;
    const size_t nn = (size_t)n_nodes + 1, ne = (size_t)n + 1;
    DevBuf* B = h->d_mrg;
    PO_TRY(ensure(h, h->d_scalars, 128));
    PO_TRY(ensure(h, B[MB_CNT], 128));
    PO_TRY(ensure(h, B[MB_RCNT], po::MERGE_BATCH * 8));
    for (int k : {MB_OUTDEG, MB_INDEG, MB_OUTE, MB_INE, MB_LINK, MB_BACK, MB_JB0, MB_JB1, MB_HOPS0, MB_HOPS1, MB_HLEN, MB_PATHK, MB_NPATH,
                  MB_NPOS, MB_LEN})
        PO_TRY(ensure(h, B[k], nn * 4));
    for (int k : {MB_WS0, MB_WS1, MB_HSUM}) PO_TRY(ensure(h, B[k], nn * 8));
    for (int k : {MB_EFLAG, MB_KEEP}) PO_TRY(ensure(h, B[k], ne));
    PO_TRY(ensure(h, B[MB_KOFF], (ne + 1) * 4));
    PO_TRY(ensure(h, B[MB_TMP], ne * sizeof(po_edge)));
    const po::Edge* d_edges = edges->d_rows.as<po::Edge>();
    const unsigned long long* nrank = edges->d_nrank.as<unsigned long long>();
    unsigned long long *cnt = B[MB_CNT].as<unsigned long long>(), *rcnt = B[MB_RCNT].as<unsigned long long>();
    uint32_t *outdeg = B[MB_OUTDEG].as<uint32_t>(), *indeg = B[MB_INDEG].as<uint32_t>(), *oute = B[MB_OUTE].as<uint32_t>(),
             *ine = B[MB_INE].as<uint32_t>(), *link = B[MB_LINK].as<uint32_t>(), *back = B[MB_BACK].as<uint32_t>(),
             *hlen = B[MB_HLEN].as<uint32_t>(), *pathk = B[MB_PATHK].as<uint32_t>(), *npath = B[MB_NPATH].as<uint32_t>(),
             *npos = B[MB_NPOS].as<uint32_t>(), *d_len = B[MB_LEN].as<uint32_t>();
    uint32_t* jb[2] = {B[MB_JB0].as<uint32_t>(), B[MB_JB1].as<uint32_t>()};
    uint32_t* hops[2] = {B[MB_HOPS0].as<uint32_t>(), B[MB_HOPS1].as<uint32_t>()};
    unsigned long long* ws[2] = {B[MB_WS0].as<unsigned long long>(), B[MB_WS1].as<unsigned long long>()};
    unsigned long long* hsum = B[MB_HSUM].as<unsigned long long>();
    uint8_t *eflag = B[MB_EFLAG].as<uint8_t>(), *keep = B[MB_KEEP].as<uint8_t>();
    uint32_t* koff = B[MB_KOFF].as<uint32_t>();
    po::Edge* renamed = B[MB_TMP].as<po::Edge>();
    const uint32_t edge_grid = stride_grid(h, n);
    const uint32_t node_blocks = std::max<uint32_t>(1u, cdiv(n_nodes, 256));
    // a head has a link out, into a node that is no head: at most every second node is one
    const uint32_t max_heads = n_nodes / 2 + 1;
    uint32_t pad_cap = 1;
    while (pad_cap < max_heads) pad_cap <<= 1;
    PO_TRY(ensure(h, B[MB_HKEY], (size_t)pad_cap * 8));
    PO_TRY(ensure(h, B[MB_HVAL], (size_t)pad_cap * 4));
    unsigned long long* hkey = B[MB_HKEY].as<unsigned long long>();
    uint32_t* hval = B[MB_HVAL].as<uint32_t>();
    // (the memsets and the lengths are work of every call: inside ms_links and ms_total.  The lengths go up again
    // because the copy po_layout_edges left on the handle is as old as that call: reads may have been added since.)
    HIP_TRY(h, hipEventRecord(ev[0], st));
    HIP_TRY(h, hipMemsetAsync(cnt, 0, 128, st));
    for (uint32_t* p : {outdeg, indeg}) HIP_TRY(h, hipMemsetAsync(p, 0, nn * 4, st));
    for (uint32_t* p : {oute, ine}) HIP_TRY(h, hipMemsetAsync(p, 0xFF, nn * 4, st));
    HIP_TRY(h, hipMemsetAsync(hkey, 0xFF, (size_t)pad_cap * 8, st));   // (the sort's padding: behind every rank word)
    if (n_nodes) HIP_TRY(h, hipMemcpyAsync(d_len, h->len.data(), (size_t)n_nodes * 4, hipMemcpyHostToDevice, st));
    if (n) {
        hipLaunchKernelGGL(po::k_merge_degree, dim3(edge_grid), dim3(256), 0, st, d_edges, n, n_nodes, outdeg, indeg, oute, ine, cnt);
        HIP_TRY(h, hipGetLastError());
    }
    HIP_TRY(h, hipMemcpyAsync(h->pinned + 16, cnt, po::MC_N * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    M.n_invalid = h->pinned[16 + po::MC_INVALID];
    // (an edge that names a node the handle does not hold would index out of the degree arrays: nothing is linked then)
    if (M.n_invalid) return fail(h, PO_ERR_INVALID, "po_layout_merge: an edge names a read the handle does not hold");
    if (n_nodes) {
        hipLaunchKernelGGL(po::k_merge_links, dim3(node_blocks), dim3(256), 0, st, d_edges, n, n_nodes, nrank, outdeg, indeg, oute, ine,
                           link, back, jb[0], hops[0], ws[0], hlen, hkey, hval, cnt);
        HIP_TRY(h, hipGetLastError());
    }
    HIP_TRY(h, hipMemcpyAsync(h->pinned + 16, cnt, po::MC_N * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipEventRecord(ev[1], st));
    HIP_TRY(h, hipStreamSynchronize(st));
    M.n_nodes = h->pinned[16 + po::MC_NODES];
    const uint64_t K64 = h->pinned[16 + po::MC_HEADS];
    if (K64 > max_heads) return fail(h, PO_ERR_HIP, "internal: po_layout_merge counted more heads than nodes allow");
    const uint32_t K = (uint32_t)K64;
    M.n_merged = K;
    if ((uint64_t)n_nodes + K > 0xFFFFFFFFull) {
        M.n_overflow = 1;
        return fail(h, PO_ERR_INVALID, "po_layout_merge: the merged nodes do not fit 32-bit node ids");
    }
    // List ranking.  A node sits fewer than n_nodes links behind its head, so ceil(log2(n_nodes)) rounds reach every
    // head; the bound is the host's (po::merge_round_cap), no kernel follows links.  Rounds go out in batches, one readback
    // per batch: round j of a batch counts the nodes that reached a root in it in word j, and the first round that counts
    // none ends the ranking (later rounds of its batch change nothing on a path).
    const uint32_t max_rounds = po::merge_round_cap(M.n_nodes);
    uint32_t launched = 0, rounds = 0;
    for (bool done = K == 0; !done && launched < max_rounds;) {
        const uint32_t batch = std::min<uint32_t>(po::MERGE_BATCH, max_rounds - launched);
        HIP_TRY(h, hipMemsetAsync(rcnt, 0, (size_t)batch * 8, st));
        for (uint32_t j = 0; j < batch; ++j, ++launched) {
            const int a = po::merge_final_buffer(launched), b = a ^ 1;
            hipLaunchKernelGGL(po::k_merge_jump, dim3(node_blocks), dim3(256), 0, st, n_nodes, back, jb[a], hops[a], ws[a], jb[b],
                               hops[b], ws[b], rcnt + j);
        }
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(h->pinned + 32, rcnt, (size_t)batch * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipStreamSynchronize(st));
        done = po::merge_rounds_done(h->pinned + 32, batch, rounds);
    }
    M.n_rounds = rounds;
    const int fin = po::merge_final_buffer(launched);   // the triple the last launch wrote
    HIP_TRY(h, hipEventRecord(ev[2], st));
    const uint32_t pad = po::merge_sort_pad(K);
    if (n_nodes) {
        hipLaunchKernelGGL(po::k_merge_tails, dim3(node_blocks), dim3(256), 0, st, n_nodes, link, back, jb[fin], hops[fin], ws[fin], hlen,
                           hsum, cnt);
        // heads by rank: bitonic sort of the K rank words, padded with all ones to a power of two
        po::merge_sort_steps(K, [&](uint32_t j, uint32_t k) {
            hipLaunchKernelGGL(po::k_merge_bitonic, dim3(cdiv(pad, 256)), dim3(256), 0, st, hkey, hval, pad, j, k);
        });
        HIP_TRY(h, hipGetLastError());
    }
    PO_TRY(ensure(h, B[MB_LENS], ((size_t)K + 1) * 4));
    PO_TRY(ensure(h, B[MB_PSUM], ((size_t)K + 1) * 8));
    PO_TRY(ensure(h, res->d_moff, std::max<size_t>(((size_t)K + 2) * 4, 256), 1.0, false));
    PO_TRY(ensure(h, res->d_mlen, std::max<size_t>((size_t)K * 8, 256), 1.0, false));
    uint32_t *lens = B[MB_LENS].as<uint32_t>(), *moff = res->d_moff.as<uint32_t>();
    long long* psum = B[MB_PSUM].as<long long>();
    if (K) {
        hipLaunchKernelGGL(po::k_merge_number, dim3(cdiv(K, 256)), dim3(256), 0, st, K, n_nodes, hval, hlen, hsum, pathk, lens, psum);
        HIP_TRY(h, hipGetLastError());
    }
    PO_TRY(prefix_sum<uint32_t>(h, lens, K, moff, &h->pinned[3]));
    HIP_TRY(h, hipMemcpyAsync(h->pinned + 16, cnt, po::MC_N * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipEventRecord(ev[3], st));
    HIP_TRY(h, hipStreamSynchronize(st));
    const uint64_t n_members = h->pinned[3];
    M.n_nodes_merged = h->pinned[16 + po::MC_MERGED];
    M.n_cycle_nodes = h->pinned[16 + po::MC_CYCLE];
    M.max_path_nodes = h->pinned[16 + po::MC_MAXPATH];
    // (every node that reached a head is a member of that head's path: the lengths the last nodes wrote add up to them)
    if (n_members != M.n_nodes_merged) return fail(h, PO_ERR_HIP, "internal: the path lengths of po_layout_merge do not add up");
    PO_TRY(ensure(h, res->d_member, std::max<size_t>(n_members * 4, 256), 1.0, false));
    PO_TRY(ensure(h, res->d_prefix, std::max<size_t>(n_members * 4, 256), 1.0, false));
    const size_t n_out_nodes = (size_t)n_nodes + K;
    const size_t nrank_bytes = std::max<size_t>(n_out_nodes * 8, 256);
    PO_TRY(ensure_nrank(h, res, nrank_bytes));
    if (n_nodes) {
        hipLaunchKernelGGL(po::k_merge_tables, dim3(node_blocks), dim3(256), 0, st, d_edges, n, n_nodes, d_len, link, back, jb[fin],
                           hops[fin], ws[fin], oute, pathk, moff, K, (uint32_t)n_members, res->d_member.as<uint32_t>(),
                           res->d_prefix.as<int32_t>(), res->d_mlen.as<long long>(), npath, npos);
        hipLaunchKernelGGL(po::k_merge_ranks, dim3(stride_grid(h, n_nodes)), dim3(256), 0, st, n_nodes, K, nrank, npath, cnt,
                           res->d_nrank.as<unsigned long long>());
        HIP_TRY(h, hipGetLastError());
    }
    PO_TRY(fill_nrank_tail(h, res, n_out_nodes, nrank_bytes));
    if (n) {
        hipLaunchKernelGGL(po::k_merge_edges, dim3(edge_grid), dim3(256), 0, st, d_edges, n, n_nodes, link, npath, psum, renamed, eflag,
                           keep, cnt);
        HIP_TRY(h, hipGetLastError());
    }
    uint64_t n_kept = 0;
    const EdgeMarks marks = {keep, eflag, koff};
    PO_TRY(stage2_count(h, n, cnt, po::MC_N, marks, flags_out != nullptr, n_kept));
    M.n_self_loops = h->pinned[16 + po::MC_SELF];
    M.n_overflow = h->pinned[16 + po::MC_OVERFLOW];
    M.n_edges_out = n_kept;
    if (M.n_overflow) return fail(h, PO_ERR_INVALID, "po_layout_merge: the weight of an edge out of a merged node does not fit 32 bits");
    PO_TRY(stage2_emit(h, res, n, n_kept, renamed, nullptr, marks, flags_out, ev[4]));
    res->n_merged = K;
    res->n_members = n_members;
    (void)hipEventElapsedTime(&M.ms_links, ev[0], ev[1]);
    (void)hipEventElapsedTime(&M.ms_rank, ev[1], ev[2]);
    (void)hipEventElapsedTime(&M.ms_number, ev[2], ev[3]);
    (void)hipEventElapsedTime(&M.ms_emit, ev[3], ev[4]);
    (void)hipEventElapsedTime(&M.ms_total, ev[0], ev[4]);
    return PO_OK;
}

// one output of po_layout_coverage, _components or _partition on its way to the caller (`dst` null: not wanted)
struct Landing {
    const void* src;
    size_t bytes;
    void* dst;
};

// The outputs through the handle's pinned landing buffer, in list order, then the first `n_counters` counters to words
// 16.. of the landing zone; one synchronise, then the copies into the caller's memory.
po_status land_outputs(po_handle* h, std::initializer_list<Landing> outs, const unsigned long long* cnt, int n_counters) {
    hipStream_t st = h->stream;
    size_t total = 16;
    for (const Landing& o : outs) total += o.bytes;
    PO_TRY(ensure_host(h, h->scratch_host, total));
    char* land = static_cast<char*>(h->scratch_host.p);
    size_t at = 0;
    for (const Landing& o : outs) {
        if (o.bytes && o.dst) HIP_TRY(h, hipMemcpyAsync(land + at, o.src, o.bytes, hipMemcpyDeviceToHost, st));
        at += o.bytes;
    }
    HIP_TRY(h, hipMemcpyAsync(h->pinned + 16, cnt, (size_t)n_counters * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    at = 0;
    for (const Landing& o : outs) {
        if (o.bytes && o.dst) std::memcpy(o.dst, land + at, o.bytes);
        at += o.bytes;
    }
    return PO_OK;
}

// ---- average_coverage_path per edge (po_layout_coverage): edges + all rows -> (read_length_sum, path_length) per edge ----

po_status run_coverage(po_handle* h, po_result* graph, po_result* rows, po_edge_coverage* out) {
    hipStream_t st = h->stream;
    po_coverage_stats& C = h->cstats;
    C = po_coverage_stats();
    const uint32_t n_ids = (uint32_t)h->len.size();
    if (graph->count >= 0x7FFFFF00ull) return fail(h, PO_ERR_CAPACITY, "po_layout_coverage: too many edges for one call");
    // (the pair table has 4 slots per row and is indexed with 32 bits)
    if (rows->count >= 0x3FFFFF00ull) return fail(h, PO_ERR_CAPACITY, "po_layout_coverage: more than 2^30 rows in one call");
    const uint32_t n = (uint32_t)graph->count, n_rows = (uint32_t)rows->count;
    C.n_edges = n;
    C.n_rows = n_rows;
    if (n == 0) return PO_OK;
    const uint32_t K = graph->merged ? (uint32_t)graph->n_merged : 0u, n_members = graph->merged ? (uint32_t)graph->n_members : 0u;
    if ((uint64_t)n_ids + K > 0xFFFFFFFEull) return fail(h, PO_ERR_CAPACITY, "po_layout_coverage: the nodes do not fit 32-bit node ids");
    const uint32_t n_total = n_ids + K;
    PO_TRY(lay_events(h));
    hipEvent_t* ev = h->ev_lay + EV_COVERAGE;
    PO_TRY(rows_to_device(h, graph));
    PO_TRY(rows_to_device(h, rows));
    const uint32_t n_slots = po::cov_table_slots(n_rows);
    const size_t nn = (size_t)n_total + 1, n_list = 2 * (size_t)n_rows + 1;
    DevBuf* B = h->d_cov;
    PO_TRY(ensure(h, h->d_scalars, 128));
    PO_TRY(ensure(h, B[VB_CNT], 128));
    for (int k : {VB_USED, VB_NODEOF, VB_LEN, VB_SETCNT, VB_OFF, VB_CUR}) PO_TRY(ensure(h, B[k], nn * 4));
    PO_TRY(ensure(h, B[VB_SUM], nn * 8));
    PO_TRY(ensure(h, B[VB_TABLE], (size_t)n_slots * 8));
    PO_TRY(ensure(h, B[VB_LIST], n_list * 4));
    PO_TRY(ensure(h, B[VB_OUT], (size_t)n * sizeof(po::EdgeCoverage)));
    unsigned long long *cnt = B[VB_CNT].as<unsigned long long>(), *table = B[VB_TABLE].as<unsigned long long>(),
                       *sum = B[VB_SUM].as<unsigned long long>();
    uint32_t *used = B[VB_USED].as<uint32_t>(), *node_of = B[VB_NODEOF].as<uint32_t>(), *d_len = B[VB_LEN].as<uint32_t>(),
             *setcnt = B[VB_SETCNT].as<uint32_t>(), *off = B[VB_OFF].as<uint32_t>(), *cur = B[VB_CUR].as<uint32_t>(),
             *list = B[VB_LIST].as<uint32_t>();
    po::EdgeCoverage* d_out = B[VB_OUT].as<po::EdgeCoverage>();
    const po::Edge* d_edges = graph->d_rows.as<po::Edge>();
    const po::Row* d_rows = rows->d_rows.as<po::Row>();
    const uint32_t cap = (uint32_t)h->n_cu * 8;
    const uint32_t edge_grid = stride_grid(h, n), row_grid = stride_grid(h, n_rows);
    const uint32_t node_blocks = std::max<uint32_t>(1u, cdiv(n_total, 256));
    // (the memsets and the lengths are work of every call: inside ms_sets and ms_total)
    HIP_TRY(h, hipEventRecord(ev[0], st));
    HIP_TRY(h, hipMemsetAsync(cnt, 0, 128, st));
    for (uint32_t* p : {used, setcnt, cur}) HIP_TRY(h, hipMemsetAsync(p, 0, nn * 4, st));
    HIP_TRY(h, hipMemsetAsync(node_of, 0xFF, nn * 4, st));
    HIP_TRY(h, hipMemsetAsync(sum, 0, nn * 8, st));
    HIP_TRY(h, hipMemsetAsync(table, 0xFF, (size_t)n_slots * 8, st));
    if (n_ids) HIP_TRY(h, hipMemcpyAsync(d_len, h->len.data(), (size_t)n_ids * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(po::k_cov_mark, dim3(edge_grid), dim3(256), 0, st, d_edges, n, n_total, used, cnt);
    hipLaunchKernelGGL(po::k_cov_nodes, dim3(node_blocks), dim3(256), 0, st, n_ids, n_total, used, node_of, cnt);
    if (n_members && K)
        hipLaunchKernelGGL(po::k_cov_members, dim3(cdiv(n_members, 256)), dim3(256), 0, st, graph->d_member.as<uint32_t>(), n_members,
                           graph->d_moff.as<uint32_t>(), K, n_ids, used, node_of, cnt);
    if (n_rows)
        hipLaunchKernelGGL(po::k_cov_insert, dim3(row_grid), dim3(256), 0, st, d_rows, n_rows, n_ids, d_len, node_of, table, n_slots, sum,
                           setcnt, cnt);
    hipLaunchKernelGGL(po::k_cov_max, dim3(std::min<uint32_t>(node_blocks, cap)), dim3(256), 0, st, setcnt, n_total, cnt);
    HIP_TRY(h, hipGetLastError());
    PO_TRY(prefix_sum<uint32_t>(h, setcnt, n_total, off, &h->pinned[2]));
    HIP_TRY(h, hipMemcpyAsync(h->pinned + 16, cnt, po::CC_N * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    C.n_invalid = h->pinned[16 + po::CC_INVALID];
    C.n_nodes = h->pinned[16 + po::CC_NODES];
    C.n_pairs = h->pinned[16 + po::CC_PAIRS];
    C.max_set = h->pinned[16 + po::CC_MAXSET];
    if (C.n_invalid) return fail(h, PO_ERR_INVALID, "po_layout_coverage: an edge or a row names a read the handle does not hold");
    if (h->pinned[2] != C.n_pairs || C.n_pairs >= n_list)
        return fail(h, PO_ERR_HIP, "internal: the set sizes of po_layout_coverage do not add up");
    const uint32_t n_pairs = (uint32_t)C.n_pairs;
    if (n_pairs)
        hipLaunchKernelGGL(po::k_cov_fill, dim3(stride_grid(h, n_slots)), dim3(256), 0, st, table, n_slots, n_total, off, cur, list,
                           n_pairs);
    HIP_TRY(h, hipEventRecord(ev[1], st));
    // one wave per edge, four to a workgroup
    hipLaunchKernelGGL(po::k_cov_edges, dim3(std::max<uint32_t>(1u, std::min<uint32_t>(cdiv(n, 4), cap * 4))), dim3(256), 0, st, d_edges,
                       n, n_ids, n_total, d_len, graph->merged ? graph->d_mlen.as<long long>() : (const long long*)nullptr, table, n_slots,
                       sum, setcnt, off, list, n_pairs, d_out, cnt);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(ev[2], st));
    PO_TRY(land_outputs(h, {{d_out, (size_t)n * sizeof(po_edge_coverage), out}}, cnt, po::CC_N));
    C.n_zero_path = h->pinned[16 + po::CC_ZERO];
    (void)hipEventElapsedTime(&C.ms_sets, ev[0], ev[1]);
    (void)hipEventElapsedTime(&C.ms_edges, ev[1], ev[2]);
    (void)hipEventElapsedTime(&C.ms_total, ev[0], ev[2]);
    return PO_OK;
}

// ---- what the analysis stages on a graph result (po_layout_components, po_layout_partition) share --------------------
// A driver resets its stats, opens with ranked_open, runs its rounds on the ranks, launches its k_*_roots, and closes with
// ranked_roots, its label kernels and land_outputs (above); it reads its own counters from words 16.. of the landing zone.

// a graph result by rank (the place of a node in the node order), as ranked_open leaves it on the device
struct RankedGraph {
    uint32_t n = 0, n_total = 0, n_order = 0, pad = 0, edge_grid = 0, rank_grid = 0;
    uint32_t *val = nullptr, *rank_of = nullptr, *index = nullptr;   // node at rank; rank of node; root number (ranked_roots)
    po::EdgeRanks* ends = nullptr;
    uint8_t* root = nullptr;
    unsigned long long *cnt = nullptr, *rcnt = nullptr;
    hipEvent_t* ev = nullptr;   // the stage's four events; null: an empty graph, nothing was launched and nothing is to do
};

// The open: the bounds, the early return of the empty graph, events, edges on the device, the shared workspaces and the
// stage's own (`own(nn, ne)` ensures them for nn node and ne edge places, `ident` among them), then the rank of every
// node -- the rank words sorted (bitonic, padded with all ones to a power of two), place r = rank r, `ident`[r] = r --
// and the two ranks of every edge, the first `n_counters` counters on the host (words 16.. of the landing zone), one
// synchronise.  Fills the n_edges, n_invalid and n_nodes of the stage's stats.
template <class Stats, class Own>
po_status ranked_open(po_handle* h, po_result* graph, const std::string& stage, int ev_first, int n_counters, Stats& S, DevBuf& ident,
                      Own&& own, RankedGraph& R) {
    hipStream_t st = h->stream;
    if (graph->count >= 0x7FFFFF00ull) return fail(h, PO_ERR_CAPACITY, stage + ": too many edges for one call");
    const uint32_t n = (uint32_t)graph->count;
    const uint64_t K = graph->merged ? graph->n_merged : 0;
    if (h->len.size() + K >= 0x7FFFFF00ull) return fail(h, PO_ERR_CAPACITY, stage + ": too many nodes for one call");
    const uint32_t n_total = (uint32_t)(h->len.size() + K);
    S.n_edges = n;
    if (n_total == 0 || !graph->d_nrank.p) {
        if (n) return fail(h, PO_ERR_INVALID, stage + ": the graph carries no node order");
        return PO_OK;
    }
    PO_TRY(lay_events(h));
    hipEvent_t* ev = h->ev_lay + ev_first;
    PO_TRY(rows_to_device(h, graph));
    const uint32_t pad = po::merge_sort_pad(n_total);
    const size_t nn = (size_t)n_total + 2, ne = (size_t)n + 1;
    DevBuf* B = h->d_rank;
    PO_TRY(ensure(h, h->d_scalars, 128));
    PO_TRY(ensure(h, B[RK_CNT], 128));
    PO_TRY(ensure(h, B[RK_RCNT], po::CC_BATCH * 8));
    PO_TRY(ensure(h, B[RK_KEY], (size_t)pad * 8));
    PO_TRY(ensure(h, B[RK_VAL], (size_t)pad * 4));
    for (int k : {RK_RANKOF, RK_INDEX}) PO_TRY(ensure(h, B[k], nn * 4));
    PO_TRY(ensure(h, B[RK_ROOT], nn));
    PO_TRY(ensure(h, B[RK_ENDS], ne * sizeof(po::EdgeRanks)));
    PO_TRY(own(nn, ne));
    R = RankedGraph{n, n_total, 0, pad, stride_grid(h, n), 0, B[RK_VAL].as<uint32_t>(), B[RK_RANKOF].as<uint32_t>(),
                    B[RK_INDEX].as<uint32_t>(), B[RK_ENDS].as<po::EdgeRanks>(), B[RK_ROOT].as<uint8_t>(),
                    B[RK_CNT].as<unsigned long long>(), B[RK_RCNT].as<unsigned long long>(), nullptr};
    unsigned long long* key = B[RK_KEY].as<unsigned long long>();
    HIP_TRY(h, hipEventRecord(ev[0], st));
    HIP_TRY(h, hipMemsetAsync(R.cnt, 0, 128, st));
    HIP_TRY(h, hipMemsetAsync(R.rank_of, 0xFF, nn * 4, st));
    hipLaunchKernelGGL(po::k_cc_keys, dim3(cdiv(pad, 256)), dim3(256), 0, st, graph->d_nrank.as<unsigned long long>(), n_total, pad, key,
                       R.val);
    po::merge_sort_steps(n_total, [&](uint32_t j, uint32_t k) {
        hipLaunchKernelGGL(po::k_merge_bitonic, dim3(cdiv(pad, 256)), dim3(256), 0, st, key, R.val, pad, j, k);
    });
    hipLaunchKernelGGL(po::k_cc_init, dim3(cdiv(pad, 256)), dim3(256), 0, st, key, R.val, pad, n_total, ident.as<uint32_t>(), R.rank_of,
                       R.cnt);
    if (n)
        hipLaunchKernelGGL(po::k_cc_ends, dim3(R.edge_grid), dim3(256), 0, st, graph->d_rows.as<po::Edge>(), n, n_total, R.rank_of, R.ends,
                           R.cnt);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(h->pinned + 16, R.cnt, (size_t)n_counters * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipEventRecord(ev[1], st));
    HIP_TRY(h, hipStreamSynchronize(st));
    S.n_invalid = h->pinned[16 + po::KC_INVALID];
    S.n_nodes = h->pinned[16 + po::KC_ORDER];
    if (S.n_invalid) return fail(h, PO_ERR_INVALID, stage + ": an edge has an end that is not in the node order");
    if (S.n_nodes > n_total) return fail(h, PO_ERR_HIP, "internal: " + stage + " counted more ranks than nodes");
    R.n_order = (uint32_t)S.n_nodes;
    R.rank_grid = stride_grid(h, R.n_order);
    R.ev = ev;
    return PO_OK;
}

// After the stage's k_*_roots: the roots numbered by rank (R.index), their number on the host.  One synchronise.
po_status ranked_roots(po_handle* h, const RankedGraph& R, const char* name, uint32_t& n_roots) {
    PO_TRY(prefix_sum<uint8_t>(h, R.root, R.n_order, R.index, &h->pinned[2]));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const uint64_t n64 = h->pinned[2];
    if (n64 > R.n_order || (R.n_order && !n64)) return fail(h, PO_ERR_HIP, std::string("internal: the roots of ") + name + " do not add up");
    n_roots = (uint32_t)n64;
    return PO_OK;
}

// what round_phase (components.hip.h) clears and reads back, on the handle's stream; the first HIP error sticks
struct RoundOps {
    po_handle* h;
    hipStream_t st;
    unsigned long long* rcnt;
    hipError_t err = hipSuccess;

    bool ok(hipError_t e) {
        if (e != hipSuccess && err == hipSuccess) err = e;
        return e == hipSuccess;
    }
    bool begin(uint32_t batch) { return ok(hipMemsetAsync(rcnt, 0, (size_t)batch * 8, st)); }
    bool end(uint32_t batch, const volatile uint64_t*& words) {
        words = h->pinned + 32;
        return ok(hipGetLastError()) && ok(hipMemcpyAsync(h->pinned + 32, rcnt, (size_t)batch * 8, hipMemcpyDeviceToHost, st)) &&
               ok(hipStreamSynchronize(st));
    }
};

// ---- weakly connected components (po_layout_components): graph result -> component per node and per edge, the table ----

po_status run_components(po_handle* h, po_result* graph, uint32_t* node_out, uint32_t* edge_out, po_component* table_out,
                         uint64_t* n_components_out) {
    hipStream_t st = h->stream;
    po_components_stats& S = h->ccstats;
    S = po_components_stats();
    DevBuf* B = h->d_cc;
    RankedGraph R;
    PO_TRY(ranked_open(h, graph, "po_layout_components", EV_COMPONENTS, po::KC_N, S, B[KB_P], [&](size_t nn, size_t ne) {
        for (int k : {KB_P, KB_COMP}) PO_TRY(ensure(h, B[k], nn * 4));
        PO_TRY(ensure(h, B[KB_TABLE], nn * sizeof(po::Component)));
        return ensure(h, B[KB_ECOMP], ne * 4);
    }, R));
    if (!R.ev) return PO_OK;
    const uint32_t n = R.n, n_order = R.n_order;
    uint32_t *p = B[KB_P].as<uint32_t>(), *comp = B[KB_COMP].as<uint32_t>(), *ecomp = B[KB_ECOMP].as<uint32_t>();
    po::Component* table = B[KB_TABLE].as<po::Component>();
    // Rounds of hook + jump in batches, one change word per round and one readback per batch; the first round that
    // lowered no word ends them (the later rounds of its batch lower nothing either).  The bound is the host's.
    if (n_order) {
        RoundOps ops{h, st, R.rcnt};
        uint64_t lowered = 0;
        const int how = po::round_phase(ops, n_order, [&](uint32_t j) {
            if (n) hipLaunchKernelGGL(po::k_cc_hook, dim3(R.edge_grid), dim3(256), 0, st, R.ends, n, n_order, p, R.rcnt + j);
            hipLaunchKernelGGL(po::k_cc_jump, dim3(R.rank_grid), dim3(256), 0, st, n_order, p, R.rcnt + j);
        }, S.n_rounds, S.n_batches, lowered);
        if (how == po::ROUNDS_FAILED) HIP_TRY(h, ops.err != hipSuccess ? ops.err : hipErrorUnknown);
        if (how != po::ROUNDS_DONE) return fail(h, PO_ERR_HIP, "internal: po_layout_components reached its bound of n_order + 2 rounds");
    }
    HIP_TRY(h, hipEventRecord(R.ev[2], st));
    if (n_order) {
        hipLaunchKernelGGL(po::k_cc_roots, dim3(R.rank_grid), dim3(256), 0, st, p, n_order, R.root);
        HIP_TRY(h, hipGetLastError());
    }
    uint32_t n_comp = 0;
    PO_TRY(ranked_roots(h, R, "po_layout_components", n_comp));
    S.n_components = n_comp;
    if (n_comp) {
        HIP_TRY(h, hipMemsetAsync(table, 0, (size_t)n_comp * sizeof(po::Component), st));
        hipLaunchKernelGGL(po::k_cc_label_nodes, dim3(R.rank_grid), dim3(256), 0, st, p, R.index, R.val, n_order, n_comp, comp, table);
        if (n) hipLaunchKernelGGL(po::k_cc_label_edges, dim3(R.edge_grid), dim3(256), 0, st, R.ends, n, n_order, n_comp, comp, ecomp, table);
        hipLaunchKernelGGL(po::k_cc_max, dim3(stride_grid(h, n_comp)), dim3(256), 0, st, table, n_comp, R.cnt);
        HIP_TRY(h, hipGetLastError());
    }
    HIP_TRY(h, hipEventRecord(R.ev[3], st));
    static_assert(sizeof(po_component) == sizeof(po::Component), "po_component is the device's table entry");
    PO_TRY(land_outputs(h, {{table, (size_t)n_comp * sizeof(po_component), table_out}, {comp, (size_t)n_order * 4, node_out},
                            {ecomp, (size_t)n * 4, edge_out}}, R.cnt, po::KC_N));
    S.n_singletons = h->pinned[16 + po::KC_SINGLE];
    S.max_component_nodes = h->pinned[16 + po::KC_MAXN];
    S.max_component_edges = h->pinned[16 + po::KC_MAXE];
    *n_components_out = n_comp;
    (void)hipEventElapsedTime(&S.ms_rounds, R.ev[1], R.ev[2]);
    (void)hipEventElapsedTime(&S.ms_label, R.ev[2], R.ev[3]);
    (void)hipEventElapsedTime(&S.ms_total, R.ev[0], R.ev[3]);
    return PO_OK;
}

// ---- strongly connected components and the superbubble partition (po_layout_partition) -----------------------------------

// what scc_drive (partition.hip.h) launches and reads back, on the handle's stream
struct SccOps : RoundOps {
    const RankedGraph& R;
    uint8_t *live, *mark, *has_in, *has_out;
    uint32_t *scc, *colour;

    void trim_round(uint32_t j) {
        if (R.n) hipLaunchKernelGGL(po::k_scc_trim_edges, dim3(R.edge_grid), dim3(256), 0, st, R.ends, R.n, R.n_order, live, has_in, has_out);
        hipLaunchKernelGGL(po::k_scc_trim_ranks, dim3(R.rank_grid), dim3(256), 0, st, R.n_order, live, scc, has_in, has_out, rcnt + j);
    }
    void colour_init() { hipLaunchKernelGGL(po::k_scc_colour_init, dim3(R.rank_grid), dim3(256), 0, st, R.n_order, live, colour, mark); }
    void forward_round(uint32_t j) {
        if (R.n) hipLaunchKernelGGL(po::k_scc_forward, dim3(R.edge_grid), dim3(256), 0, st, R.ends, R.n, R.n_order, live, colour, rcnt + j);
    }
    void back_init() { hipLaunchKernelGGL(po::k_scc_back_init, dim3(R.rank_grid), dim3(256), 0, st, R.n_order, live, colour, mark); }
    void backward_round(uint32_t j) {
        if (R.n)
            hipLaunchKernelGGL(po::k_scc_backward, dim3(R.edge_grid), dim3(256), 0, st, R.ends, R.n, R.n_order, live, colour, mark, rcnt + j);
    }
    bool retire(uint64_t& retired) {
        if (!ok(hipMemsetAsync(rcnt, 0, 8, st))) return false;
        hipLaunchKernelGGL(po::k_scc_retire, dim3(R.rank_grid), dim3(256), 0, st, R.n_order, live, colour, mark, scc, rcnt);
        if (!ok(hipGetLastError()) || !ok(hipMemcpyAsync(h->pinned + 40, rcnt, 8, hipMemcpyDeviceToHost, st)) || !ok(hipStreamSynchronize(st)))
            return false;
        retired = h->pinned[40];
        return true;
    }
};

// The SCC stage on the device, as po_layout_partition and po_layout_superbubbles run it (`name`, the first of the caller's
// events, the caller's stats): ranked_open with the workspaces of d_scc and the caller's `own`, the rounds of scc_drive,
// the numbering of the roots, the table, the class byte per edge and the flag byte per rank, all left in d_scc; the
// counters in R.cnt.  Records R.ev[2] behind the rounds.  W is filled whatever the outcome.  !R.ev: nothing to do.
// scc_rounds is everything behind the open, on whatever ranks and edge ends R names (po_layout_superbubbles_all: a flat graph).
po_status scc_rounds(po_handle* h, const std::string& name, const RankedGraph& R, po::SccWork& W, uint32_t& n_scc) {
    hipStream_t st = h->stream;
    DevBuf* B = h->d_scc;
    const uint32_t n = R.n, n_order = R.n_order;
    uint32_t *scc = B[PB_SCC].as<uint32_t>(), *colour = B[PB_COLOUR].as<uint32_t>(), *node_scc = B[PB_NODESCC].as<uint32_t>(),
             *flagw = B[PB_FLAGW].as<uint32_t>();
    uint8_t *live = B[PB_LIVE].as<uint8_t>(), *mark = B[PB_MARK].as<uint8_t>(), *has_in = B[PB_HASIN].as<uint8_t>(),
            *has_out = B[PB_HASOUT].as<uint8_t>(), *flags = B[PB_FLAGS].as<uint8_t>(), *eclass = B[PB_ECLASS].as<uint8_t>();
    po::Scc* table = B[PB_TABLE].as<po::Scc>();
    // trim rounds, forward colouring, backward marking, again while live ranks remain: every bound is scc_drive's
    if (n_order) {
        hipLaunchKernelGGL(po::k_scc_init, dim3(R.rank_grid), dim3(256), 0, st, n_order, live, scc, has_in, has_out);
        SccOps ops{{h, st, R.rcnt}, R, live, mark, has_in, has_out, scc, colour};
        const int how = po::scc_drive(ops, n_order, W);
        if (how == po::SCC_FAILED) HIP_TRY(h, ops.err != hipSuccess ? ops.err : hipErrorUnknown);
        if (how == po::SCC_ROUND_CAP) return fail(h, PO_ERR_HIP, "internal: a phase of " + name + " reached its bound of live + 2 rounds");
        if (how == po::SCC_OUTER_CAP) return fail(h, PO_ERR_HIP, "internal: " + name + " reached its bound of n_order iterations");
        if (how != po::SCC_DONE) return fail(h, PO_ERR_HIP, "internal: the live nodes of " + name + " do not add up");
    }
    HIP_TRY(h, hipEventRecord(R.ev[2], st));
    if (n_order) {
        hipLaunchKernelGGL(po::k_scc_roots, dim3(R.rank_grid), dim3(256), 0, st, scc, n_order, R.root, flagw);
        HIP_TRY(h, hipGetLastError());
    }
    PO_TRY(ranked_roots(h, R, name.c_str(), n_scc));
    if (n_scc) {
        HIP_TRY(h, hipMemsetAsync(table, 0, (size_t)n_scc * sizeof(po::Scc), st));
        hipLaunchKernelGGL(po::k_scc_label_nodes, dim3(R.rank_grid), dim3(256), 0, st, scc, R.index, R.val, n_order, n_scc, node_scc, table);
        if (n)
            hipLaunchKernelGGL(po::k_scc_edges, dim3(R.edge_grid), dim3(256), 0, st, R.ends, n, n_order, n_scc, node_scc, table, eclass, flagw,
                               R.cnt);
        hipLaunchKernelGGL(po::k_scc_flags, dim3(R.rank_grid), dim3(256), 0, st, n_order, n_scc, node_scc, flagw, table, flags);
        hipLaunchKernelGGL(po::k_scc_max, dim3(stride_grid(h, n_scc)), dim3(256), 0, st, table, n_scc, R.cnt);
        HIP_TRY(h, hipGetLastError());
    }
    return PO_OK;
}

template <class Stats, class Own>
po_status scc_stage(po_handle* h, po_result* graph, const std::string& name, int ev_first, Stats& S, Own&& own, RankedGraph& R,
                    po::SccWork& W, uint32_t& n_scc) {
    DevBuf* B = h->d_scc;
    // (the identity words land in `colour`: colour[r] = r is where the first forward phase starts anyway)
    PO_TRY(ranked_open(h, graph, name, ev_first, po::PC_N, S, B[PB_COLOUR], [&](size_t nn, size_t ne) {
        for (int k : {PB_SCC, PB_COLOUR, PB_NODESCC, PB_FLAGW}) PO_TRY(ensure(h, B[k], nn * 4));
        for (int k : {PB_LIVE, PB_MARK, PB_HASIN, PB_HASOUT, PB_FLAGS}) PO_TRY(ensure(h, B[k], nn));
        PO_TRY(ensure(h, B[PB_TABLE], nn * sizeof(po::Scc)));
        PO_TRY(ensure(h, B[PB_ECLASS], ne));
        return own(nn, ne);
    }, R));
    if (!R.ev) return PO_OK;
    return scc_rounds(h, name, R, W, n_scc);
}

po_status run_partition(po_handle* h, po_result* graph, uint32_t* node_out, uint8_t* flags_out, uint8_t* class_out, po_scc* table_out,
                        uint64_t* n_sccs_out) {
    po_partition_stats& S = h->pstats;
    S = po_partition_stats();
    DevBuf* B = h->d_scc;
    RankedGraph R;
    po::SccWork W;
    uint32_t n_scc = 0;
    const po_status staged = scc_stage(h, graph, "po_layout_partition", EV_PARTITION, S, [](size_t, size_t) { return PO_OK; }, R, W, n_scc);
    S.n_trimmed = W.n_trimmed;
    S.n_outer = W.outer;
    S.n_trim_rounds = W.trim_rounds;
    S.n_forward_rounds = W.forward_rounds;
    S.n_backward_rounds = W.backward_rounds;
    S.n_batches = W.batches;
    PO_TRY(staged);
    if (!R.ev) return PO_OK;
    const uint32_t n = R.n, n_order = R.n_order;
    S.n_sccs = n_scc;
    HIP_TRY(h, hipEventRecord(R.ev[3], h->stream));
    static_assert(sizeof(po_scc) == sizeof(po::Scc) && sizeof(po_scc) == 24, "po_scc is the device's table entry");
    PO_TRY(land_outputs(h, {{B[PB_TABLE].p, (size_t)n_scc * sizeof(po_scc), table_out}, {B[PB_NODESCC].p, (size_t)n_order * 4, node_out},
                            {B[PB_FLAGS].p, n_order, flags_out}, {B[PB_ECLASS].p, n, class_out}}, R.cnt, po::PC_N));
    S.n_singletons = h->pinned[16 + po::PC_SINGLE];
    S.n_nonsingleton_sccs = S.n_sccs - S.n_singletons;
    S.max_scc_nodes = h->pinned[16 + po::PC_MAXN];
    S.max_scc_edges = h->pinned[16 + po::PC_MAXE];
    S.n_self_loops = h->pinned[16 + po::PC_SELF];
    for (int k = 0; k < 5; ++k) S.n_class[k] = h->pinned[16 + po::PC_CLASS + k];
    *n_sccs_out = n_scc;
    (void)hipEventElapsedTime(&S.ms_ranks, R.ev[0], R.ev[1]);
    (void)hipEventElapsedTime(&S.ms_rounds, R.ev[1], R.ev[2]);
    (void)hipEventElapsedTime(&S.ms_label, R.ev[2], R.ev[3]);
    (void)hipEventElapsedTime(&S.ms_total, R.ev[0], R.ev[3]);
    return PO_OK;
}

// ---- the superbubbles of the acyclic partitions (po_layout_superbubbles, superbubbles.hip.h) ------------------------------

// what the superbubble stage counts, for the stats of its callers
struct SbWork {
    uint64_t n_p_nodes = 0, n_p_edges = 0, n_bubbles = 0, n_nested = 0, n_self_loop_nodes = 0, n_discarded = 0;
    uint32_t n_levels_forward = 0, n_levels_backward = 0, n_scc_rounds = 0, n_level_rounds = 0, n_discard_rounds = 0, n_batches = 0;
};

template <class Seed>
po_status superbubble_dag(po_handle* h, const char* const name, const RankedGraph& R, uint32_t n_scc, SbWork& S, Seed&& seed);

// The superbubble stage on the device, as po_layout_superbubbles and po_layout_bubblechains run it (`name`, the first of
// the caller's events, the caller's stats for ranked_open): scc_stage with the workspaces of d_sb and the caller's `own`,
// then everything up to the table, all left in d_sb -- the byte "enters a surviving bubble" per rank in R.root, the number
// of every entrance in R.index, exit_of in UB_EXIT, the holder in UB_INSIDE; the counters in UB_CNT.  Records ev[3]..ev[6].
// S is filled whatever the outcome.  !R.ev or !R.n_order: nothing to do.
template <class Stats, class Own>
po_status superbubble_stage(po_handle* h, po_result* graph, const char* const name, int ev_first, Stats& stats, Own&& own, RankedGraph& R,
                            SbWork& S) {
    DevBuf* B = h->d_sb;
    po::SccWork W;
    uint32_t n_scc = 0;
    const po_status staged = scc_stage(h, graph, name, ev_first, stats, [&](size_t nn, size_t ne) {
        PO_TRY(ensure(h, B[UB_CNT], 128));
        for (int k : {UB_W, UB_CIN, UB_COUT, UB_OFFIN, UB_OFFOUT, UB_CURIN, UB_CUROUT, UB_LVLF, UB_LVLB, UB_IDOM, UB_IPDOM, UB_DEPTH, UB_EXIT,
                      UB_ENCL, UB_INSIDE, UB_TOTAL, UB_EXITOUT, UB_INSIDEOUT})
            PO_TRY(ensure(h, B[k], nn * 4));
        for (int k : {UB_DEAD, UB_FLAGSOUT}) PO_TRY(ensure(h, B[k], nn));
        for (int k : {UB_LISTIN, UB_LISTOUT}) PO_TRY(ensure(h, B[k], ne * 4));
        PO_TRY(ensure(h, B[UB_TABLE], nn * sizeof(po::Bubble)));
        return own(nn, ne);
    }, R, W, n_scc);
    S.n_scc_rounds = W.trim_rounds + W.forward_rounds + W.backward_rounds;
    S.n_batches = W.batches;
    PO_TRY(staged);
    if (!R.ev || !R.n_order) return PO_OK;
    HIP_TRY(h, hipEventRecord(R.ev[3], h->stream));
    return superbubble_dag(h, name, R, n_scc, S, [] { return false; });
}

// Everything behind the SCC stage, on whatever ranks and edge ends R names (po_layout_superbubbles_all: a flat graph), with
// the SCCs, classes and flags that scc_rounds left in d_scc for them.  seed() may mark bubbles dead before the discard rounds
// (it runs behind k_sb_encl; true: it launched something, so the rounds run even without a self-loop).
template <class Seed>
po_status superbubble_dag(po_handle* h, const char* const name, const RankedGraph& R, uint32_t n_scc, SbWork& S, Seed&& seed) {
    hipStream_t st = h->stream;
    DevBuf* B = h->d_sb;
    const uint32_t n = R.n, n_order = R.n_order;
    hipEvent_t* ev = R.ev;
    unsigned long long* cnt = B[UB_CNT].as<unsigned long long>();
    uint32_t *w = B[UB_W].as<uint32_t>(), *cin = B[UB_CIN].as<uint32_t>(), *cout = B[UB_COUT].as<uint32_t>(),
             *off_in = B[UB_OFFIN].as<uint32_t>(), *off_out = B[UB_OFFOUT].as<uint32_t>(), *cur_in = B[UB_CURIN].as<uint32_t>(),
             *cur_out = B[UB_CUROUT].as<uint32_t>(), *list_in = B[UB_LISTIN].as<uint32_t>(), *list_out = B[UB_LISTOUT].as<uint32_t>(),
             *lvl_f = B[UB_LVLF].as<uint32_t>(), *lvl_b = B[UB_LVLB].as<uint32_t>(), *idom = B[UB_IDOM].as<uint32_t>(),
             *ipdom = B[UB_IPDOM].as<uint32_t>(), *depth = B[UB_DEPTH].as<uint32_t>(), *exit_of = B[UB_EXIT].as<uint32_t>(),
             *encl = B[UB_ENCL].as<uint32_t>(), *inside = B[UB_INSIDE].as<uint32_t>(), *total = B[UB_TOTAL].as<uint32_t>(),
             *d_exit = B[UB_EXITOUT].as<uint32_t>(), *d_inside = B[UB_INSIDEOUT].as<uint32_t>();
    uint8_t *dead = B[UB_DEAD].as<uint8_t>(), *d_flags = B[UB_FLAGSOUT].as<uint8_t>();
    po::Bubble* table = B[UB_TABLE].as<po::Bubble>();
    const uint8_t *eclass = h->d_scc[PB_ECLASS].as<uint8_t>(), *pflags = h->d_scc[PB_FLAGS].as<uint8_t>();
    volatile uint64_t* C = h->pinned + 48;   // this stage's counters on the host (words 16.. and 32.. are the scaffold's)
    auto counters_home = [&]() -> po_status {
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(h->pinned + 48, cnt, po::BC_N * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipStreamSynchronize(st));
        return PO_OK;
    };
    // the structure graph D: degrees, the parents and the children of every rank, sources and sinks
    HIP_TRY(h, hipMemsetAsync(cnt, 0, 128, st));
    hipLaunchKernelGGL(po::k_sb_init, dim3(stride_grid(h, (uint64_t)n_order + 1)), dim3(256), 0, st, n_order, n_scc,
                       h->d_scc[PB_NODESCC].as<uint32_t>(), h->d_scc[PB_TABLE].as<po::Scc>(), w, cin, cout, idom, ipdom, depth, exit_of, encl, total,
                       dead);
    if (n) hipLaunchKernelGGL(po::k_sb_degrees, dim3(R.edge_grid), dim3(256), 0, st, R.ends, n, n_order, eclass, w, cin, cout, cnt);
    HIP_TRY(h, hipGetLastError());
    PO_TRY(prefix_sum<uint32_t>(h, cin, n_order, off_in, &h->pinned[2]));
    PO_TRY(prefix_sum<uint32_t>(h, cout, n_order, off_out, &h->pinned[3]));
    for (uint32_t* p : {cur_in, cur_out}) HIP_TRY(h, hipMemsetAsync(p, 0, (size_t)n_order * 4, st));
    if (n)
        hipLaunchKernelGGL(po::k_sb_fill, dim3(R.edge_grid), dim3(256), 0, st, R.ends, n, n_order, eclass, cin, cout, off_in, off_out, cur_in,
                           cur_out, list_in, list_out);
    hipLaunchKernelGGL(po::k_sb_nodes, dim3(R.rank_grid), dim3(256), 0, st, n_order, pflags, cin, cout, w, lvl_f, lvl_b, cnt);
    PO_TRY(counters_home());
    const uint64_t n_real = C[po::BC_REAL], n_dedges = C[po::BC_DEDGES];
    if (h->pinned[2] != n_dedges || h->pinned[3] != n_dedges || n_dedges > n || n_real > n_order)
        return fail(h, PO_ERR_HIP, std::string("internal: the degrees of ") + name + " do not add up");
    S.n_self_loop_nodes = C[po::BC_LOOPS];
    S.n_p_nodes = n_real + (C[po::BC_R_EDGES] != 0) + (C[po::BC_RE_EDGES] != 0);
    S.n_p_edges = n_dedges + C[po::BC_LOOPS] + C[po::BC_R_EDGES] + C[po::BC_RE_EDGES];
    // the longest-path levels from the sources and from the sinks: rounds over the edges of D, bounded by round_phase
    RoundOps ops{h, st, R.rcnt};
    uint64_t ignored = 0;
    int how = po::round_phase(ops, n_real, [&](uint32_t j) {
        if (n) hipLaunchKernelGGL(po::k_sb_level, dim3(R.edge_grid), dim3(256), 0, st, R.ends, n, n_order, eclass, lvl_f, lvl_b, R.rcnt + j);
    }, S.n_level_rounds, S.n_batches, ignored);
    if (how == po::ROUNDS_FAILED) HIP_TRY(h, ops.err != hipSuccess ? ops.err : hipErrorUnknown);
    if (how != po::ROUNDS_DONE) return fail(h, PO_ERR_HIP, std::string("internal: the levels of ") + name + " reached their bound of live + 2 rounds");
    hipLaunchKernelGGL(po::k_sb_level_max, dim3(R.rank_grid), dim3(256), 0, st, n_order, lvl_f, lvl_b, cnt);
    PO_TRY(counters_home());
    const uint64_t levels_f = C[po::BC_LEVF], levels_b = C[po::BC_LEVB];
    if (levels_f > n_real || levels_b > n_real)   // (a level is the number of ranks on a path)
        return fail(h, PO_ERR_HIP, std::string("internal: ") + name + " counted more levels than nodes");
    S.n_levels_forward = (uint32_t)levels_f;
    S.n_levels_backward = (uint32_t)levels_b;
    HIP_TRY(h, hipEventRecord(ev[4], st));
    // the dominator tree and the post-dominator tree, one launch per level; the pairs; the innermost enclosing bubble
    for (uint32_t l = 1; l <= levels_f; ++l)
        hipLaunchKernelGGL(po::k_sb_tree, dim3(R.rank_grid), dim3(256), 0, st, n_order, n, l, lvl_f, off_in, cin, list_in, w,
                           (uint32_t)po::SBW_SOURCE, idom, depth, cnt);
    for (uint32_t l = 1; l <= levels_b; ++l)
        hipLaunchKernelGGL(po::k_sb_tree, dim3(R.rank_grid), dim3(256), 0, st, n_order, n, l, lvl_b, off_out, cout, list_out, w,
                           (uint32_t)po::SBW_SINK, ipdom, depth, cnt);
    hipLaunchKernelGGL(po::k_sb_pairs, dim3(R.rank_grid), dim3(256), 0, st, n_order, w, idom, ipdom, exit_of);
    for (uint32_t l = 1; l <= levels_f; ++l)
        hipLaunchKernelGGL(po::k_sb_encl, dim3(R.rank_grid), dim3(256), 0, st, n_order, l, lvl_f, idom, exit_of, encl);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(ev[5], st));
    // self-loops discard bubbles, and a discarded bubble the one around it: rounds, bounded by round_phase
    const bool seeded = seed();
    if (S.n_self_loop_nodes) hipLaunchKernelGGL(po::k_sb_dead_init, dim3(R.rank_grid), dim3(256), 0, st, n_order, w, idom, exit_of, encl, dead);
    if (S.n_self_loop_nodes || seeded) {
        how = po::round_phase(ops, n_real, [&](uint32_t j) {
            hipLaunchKernelGGL(po::k_sb_dead_round, dim3(R.rank_grid), dim3(256), 0, st, n_order, exit_of, encl, dead, R.rcnt + j);
        }, S.n_discard_rounds, S.n_batches, ignored);
        if (how == po::ROUNDS_FAILED) HIP_TRY(h, ops.err != hipSuccess ? ops.err : hipErrorUnknown);
        if (how != po::ROUNDS_DONE)
            return fail(h, PO_ERR_HIP, std::string("internal: the discards of ") + name + " reached their bound of live + 2 rounds");
    }
    hipLaunchKernelGGL(po::k_sb_label, dim3(R.rank_grid), dim3(256), 0, st, n_order, R.val, w, idom, exit_of, encl, dead, inside, total, R.root,
                       d_exit, d_inside, d_flags, cnt);
    HIP_TRY(h, hipGetLastError());
    PO_TRY(prefix_sum<uint8_t>(h, R.root, n_order, R.index, &h->pinned[2]));
    PO_TRY(counters_home());
    if (C[po::BC_WALK]) return fail(h, PO_ERR_HIP, std::string("internal: a walk along a dominator tree of ") + name + " reached its bound");
    const uint64_t n64 = h->pinned[2];
    if (n64 > n_real || C[po::BC_NESTED] > n64) return fail(h, PO_ERR_HIP, std::string("internal: the bubbles of ") + name + " do not add up");
    const uint32_t n_bubbles = (uint32_t)n64;
    S.n_bubbles = n_bubbles;
    S.n_nested = C[po::BC_NESTED];
    S.n_discarded = C[po::BC_DISCARDED];
    if (S.n_nested)
        for (uint32_t l = (uint32_t)levels_f; l >= 1; --l)
            hipLaunchKernelGGL(po::k_sb_sum, dim3(R.rank_grid), dim3(256), 0, st, n_order, l, lvl_f, R.root, inside, total);
    if (n_bubbles)
        hipLaunchKernelGGL(po::k_sb_table, dim3(R.rank_grid), dim3(256), 0, st, n_order, n_bubbles, R.val, R.root, R.index, exit_of, inside, total,
                           table);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(ev[6], st));
    return PO_OK;
}

po_status run_superbubbles(po_handle* h, po_result* graph, uint32_t* exit_out, uint32_t* inside_out, uint8_t* flags_out,
                           po_superbubble* table_out, uint64_t* n_bubbles_out) {
    po_superbubble_stats& S = h->sbstats;
    S = po_superbubble_stats();
    DevBuf* B = h->d_sb;
    RankedGraph R;
    SbWork W;
    const po_status staged = superbubble_stage(h, graph, "po_layout_superbubbles", EV_SUPERBUBBLES, S, [](size_t, size_t) { return PO_OK; }, R, W);
    S.n_p_nodes = W.n_p_nodes;
    S.n_p_edges = W.n_p_edges;
    S.n_bubbles = W.n_bubbles;
    S.n_nested = W.n_nested;
    S.n_self_loop_nodes = W.n_self_loop_nodes;
    S.n_discarded = W.n_discarded;
    S.n_levels_forward = W.n_levels_forward;
    S.n_levels_backward = W.n_levels_backward;
    S.n_scc_rounds = W.n_scc_rounds;
    S.n_level_rounds = W.n_level_rounds;
    S.n_discard_rounds = W.n_discard_rounds;
    S.n_batches = W.n_batches;
    PO_TRY(staged);
    if (!R.ev || !R.n_order) return PO_OK;
    const uint32_t n_order = R.n_order, n_bubbles = (uint32_t)W.n_bubbles;
    hipEvent_t* ev = R.ev;
    static_assert(sizeof(po_superbubble) == sizeof(po::Bubble) && sizeof(po_superbubble) == 16, "po_superbubble is the device's table entry");
    PO_TRY(land_outputs(h, {{B[UB_TABLE].p, (size_t)n_bubbles * sizeof(po_superbubble), table_out},
                            {B[UB_EXITOUT].p, (size_t)n_order * 4, exit_out}, {B[UB_INSIDEOUT].p, (size_t)n_order * 4, inside_out},
                            {B[UB_FLAGSOUT].p, n_order, flags_out}}, B[UB_CNT].as<unsigned long long>(), po::BC_N));
    *n_bubbles_out = n_bubbles;
    (void)hipEventElapsedTime(&S.ms_partition, ev[0], ev[3]);
    (void)hipEventElapsedTime(&S.ms_levels, ev[3], ev[4]);
    (void)hipEventElapsedTime(&S.ms_dominators, ev[4], ev[5]);
    (void)hipEventElapsedTime(&S.ms_label, ev[5], ev[6]);
    (void)hipEventElapsedTime(&S.ms_total, ev[0], ev[6]);
    return PO_OK;
}

// ---- the superbubbles of the whole graph, the cyclic partitions included (po_layout_superbubbles_all, cyclic.hip.h) -------

// Root splitting.  A RUN builds, level by level, a flat graph without a non-singleton SCC -- the SCC
// stage on the current flat graph (scc_rounds), one more split rank per SCC that is left -- and finds its superbubbles with
// superbubble_dag; the pairs come back by original rank and are merged into the words of d_cy.  One run suffices unless an
// SCC is rootless and its lowest rank is not certified; then the nodes of one shortest cycle through that rank root further
// runs, up to the first certified one.  The levels are bounded by n_order + 2, the runs by the longest of those cycles.
//
// The stage, as po_layout_superbubbles_all, po_layout_bubblechains_all and po_layout_contigs_all run it (`name`, the first of
// the caller's ten events, the caller's stats for ranked_open, the caller's `own` workspaces): everything up to the table,
// left per ORIGINAL rank -- the byte "enters a surviving bubble" in YB_MROOT, exit_of in YB_MEXIT, the holder in YB_MINSIDE,
// n_inside in YB_MTOTAL, the number of every entrance in R.index, the three outputs by rank and the table in d_sb; the
// counters in YB_CNT, not yet on the host (superbubble_all_counts).  Records ev[9] behind the table.  S is filled whatever
// the outcome.  !R.ev or !R.n_order: nothing to do.
template <class Stats, class Own>
po_status superbubble_all_stage(po_handle* h, po_result* graph, const char* const name, int ev_first, Stats& stats, Own&& own, RankedGraph& R,
                                po_superbubble_all_stats& S) {
    hipStream_t st = h->stream;
    DevBuf *Y = h->d_cy, *P = h->d_scc, *U = h->d_sb, *K = h->d_rank;
    PO_TRY(ranked_open(h, graph, name, ev_first, po::PC_N, stats, P[PB_COLOUR], [&](size_t nn, size_t ne) {
        const size_t n2 = 2 * nn;   // (a flat graph has at most twice the ranks)
        for (int k : {RK_INDEX}) PO_TRY(ensure(h, K[k], n2 * 4));
        PO_TRY(ensure(h, K[RK_ROOT], n2));
        for (int k : {PB_SCC, PB_COLOUR, PB_NODESCC, PB_FLAGW}) PO_TRY(ensure(h, P[k], n2 * 4));
        for (int k : {PB_LIVE, PB_MARK, PB_HASIN, PB_HASOUT, PB_FLAGS}) PO_TRY(ensure(h, P[k], n2));
        PO_TRY(ensure(h, P[PB_TABLE], n2 * sizeof(po::Scc)));
        PO_TRY(ensure(h, P[PB_ECLASS], ne));
        PO_TRY(ensure(h, U[UB_CNT], 128));
        for (int k : {UB_W, UB_CIN, UB_COUT, UB_OFFIN, UB_OFFOUT, UB_CURIN, UB_CUROUT, UB_LVLF, UB_LVLB, UB_IDOM, UB_IPDOM, UB_DEPTH, UB_EXIT,
                      UB_ENCL, UB_INSIDE, UB_TOTAL, UB_EXITOUT, UB_INSIDEOUT})
            PO_TRY(ensure(h, U[k], n2 * 4));
        for (int k : {UB_DEAD, UB_FLAGSOUT}) PO_TRY(ensure(h, U[k], n2));
        for (int k : {UB_LISTIN, UB_LISTOUT}) PO_TRY(ensure(h, U[k], ne * 4));
        PO_TRY(ensure(h, U[UB_TABLE], n2 * sizeof(po::Bubble)));
        PO_TRY(ensure(h, Y[YB_CNT], 128));
        for (int k : {YB_SIDX, YB_ROOTOF, YB_SCC0, YB_MEXIT, YB_MINSIDE, YB_MSIZE, YB_MTOTAL, YB_DIST, YB_PAR, YB_DIN, YB_PIN})
            PO_TRY(ensure(h, Y[k], nn * 4));
        for (int k : {YB_SPLIT, YB_CYCLIC0, YB_ROOTLESS, YB_UNCERTAIN, YB_ISROOT, YB_FILTERED, YB_LOOP, YB_MISEXIT, YB_MFILTERED, YB_MROOT})
            PO_TRY(ensure(h, Y[k], nn));
        for (int k : {YB_NODE, YB_ORIG, YB_BESTIN, YB_BESTOUT, YB_BESTLOW}) PO_TRY(ensure(h, Y[k], n2 * 4));
        PO_TRY(ensure(h, Y[YB_FLAT], ne * sizeof(po::EdgeRanks)));
        return own(nn, ne);
    }, R));
    if (!R.ev || !R.n_order) return PO_OK;
    R.root = K[RK_ROOT].as<uint8_t>();   // (both grew behind ranked_open's own sizes)
    R.index = K[RK_INDEX].as<uint32_t>();
    const uint32_t n = R.n, n0 = R.n_order;
    hipEvent_t* ev = R.ev;
    unsigned long long* cnt = Y[YB_CNT].as<unsigned long long>();
    uint32_t *sidx = Y[YB_SIDX].as<uint32_t>(), *root_of = Y[YB_ROOTOF].as<uint32_t>(), *scc0 = Y[YB_SCC0].as<uint32_t>(),
             *m_exit = Y[YB_MEXIT].as<uint32_t>(), *m_inside = Y[YB_MINSIDE].as<uint32_t>(), *m_size = Y[YB_MSIZE].as<uint32_t>(),
             *m_total = Y[YB_MTOTAL].as<uint32_t>(), *dist = Y[YB_DIST].as<uint32_t>(), *par = Y[YB_PAR].as<uint32_t>(),
             *din = Y[YB_DIN].as<uint32_t>(), *pin = Y[YB_PIN].as<uint32_t>(), *flat_node = Y[YB_NODE].as<uint32_t>(),
             *orig = Y[YB_ORIG].as<uint32_t>(), *best_in = Y[YB_BESTIN].as<uint32_t>(), *best_out = Y[YB_BESTOUT].as<uint32_t>(),
             *best_low = Y[YB_BESTLOW].as<uint32_t>();
    uint8_t *split = Y[YB_SPLIT].as<uint8_t>(), *cyclic0 = Y[YB_CYCLIC0].as<uint8_t>(), *rootless = Y[YB_ROOTLESS].as<uint8_t>(),
            *uncertain = Y[YB_UNCERTAIN].as<uint8_t>(), *is_root = Y[YB_ISROOT].as<uint8_t>(), *filtered = Y[YB_FILTERED].as<uint8_t>(),
            *loop = Y[YB_LOOP].as<uint8_t>(), *m_is_exit = Y[YB_MISEXIT].as<uint8_t>(), *m_filtered = Y[YB_MFILTERED].as<uint8_t>(),
            *m_root = Y[YB_MROOT].as<uint8_t>();
    po::EdgeRanks* flat = Y[YB_FLAT].as<po::EdgeRanks>();
    const uint32_t *node_scc = P[PB_NODESCC].as<uint32_t>(), *scc = P[PB_SCC].as<uint32_t>();
    const po::Scc* scc_table = P[PB_TABLE].as<po::Scc>();
    const uint8_t* pflags = P[PB_FLAGS].as<uint8_t>();
    uint32_t *exit_of = U[UB_EXIT].as<uint32_t>(), *inside = U[UB_INSIDE].as<uint32_t>(), *total = U[UB_TOTAL].as<uint32_t>();
    uint8_t* dead = U[UB_DEAD].as<uint8_t>();
    volatile uint64_t* C = h->pinned + 96;   // this call's counters on the host
    auto counters_home = [&]() -> po_status {
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(h->pinned + 16, R.cnt, po::PC_N * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipMemcpyAsync(h->pinned + 96, cnt, po::YC_N * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipStreamSynchronize(st));
        return PO_OK;
    };
    // the merged words, the self-loops, every rootless SCC's first root: its lowest rank
    HIP_TRY(h, hipMemsetAsync(cnt, 0, 128, st));
    for (uint32_t* p : {m_exit, m_inside, m_size, m_total}) HIP_TRY(h, hipMemsetAsync(p, 0xFF, (size_t)n0 * 4, st));
    for (uint8_t* p : {loop, m_is_exit, m_filtered, rootless}) HIP_TRY(h, hipMemsetAsync(p, 0, n0, st));
    if (n) hipLaunchKernelGGL(po::k_cy_loops, dim3(R.edge_grid), dim3(256), 0, st, R.ends, n, n0, loop);
    HIP_TRY(h, hipGetLastError());
    std::vector<uint32_t> roots(n0);
    for (uint32_t r = 0; r < n0; ++r) roots[r] = r;
    struct Rootless {
        uint32_t low;
        std::vector<uint32_t> cycle;   // the nodes behind `low` on one shortest cycle through it, forward
        bool done;
    };
    std::vector<Rootless> open_sccs;
    std::vector<uint8_t> bytes_a(n0), bytes_b(n0);
    float ms_split = 0, ms_bubbles = 0, ms_merge = 0;
    for (uint32_t run = 0;; ++run) {
        HIP_TRY(h, hipEventRecord(ev[7], st));
        HIP_TRY(h, hipMemcpyAsync(root_of, roots.data(), (size_t)n0 * 4, hipMemcpyHostToDevice, st));
        for (uint8_t* p : {split, uncertain, filtered}) HIP_TRY(h, hipMemsetAsync(p, 0, n0, st));
        // the levels: the flat graph of the ranks split so far, its SCCs, one more split rank per non-singleton SCC
        RankedGraph F = R;
        uint32_t n_split = 0, n_scc = 0;
        for (uint32_t level = 0;; ++level) {
            if (level > (uint64_t)n0 + 1) return fail(h, PO_ERR_HIP, std::string("internal: ") + name + " reached its bound of n_order + 2 split levels");
            const uint32_t n_flat = n0 + n_split;
            PO_TRY(prefix_sum<uint8_t>(h, split, n0, sidx, &h->pinned[4]));
            if (n) hipLaunchKernelGGL(po::k_cy_flat, dim3(R.edge_grid), dim3(256), 0, st, R.ends, n, n0, split, sidx, n_split, flat);
            hipLaunchKernelGGL(po::k_cy_ranks, dim3(R.rank_grid), dim3(256), 0, st, n0, R.val, split, sidx, n_split, flat_node, orig);
            HIP_TRY(h, hipMemsetAsync(R.cnt, 0, 128, st));
            F.ends = flat;
            F.val = flat_node;
            F.n_order = n_flat;
            F.rank_grid = stride_grid(h, n_flat);
            po::SccWork W;
            const po_status staged = scc_rounds(h, name, F, W, n_scc);
            S.n_scc_rounds += W.trim_rounds + W.forward_rounds + W.backward_rounds;
            S.n_batches += W.batches;
            PO_TRY(staged);
            if (h->pinned[4] != n_split) return fail(h, PO_ERR_HIP, std::string("internal: the split ranks of ") + name + " do not add up");
            if (level == 0) hipLaunchKernelGGL(po::k_cy_level0, dim3(R.rank_grid), dim3(256), 0, st, n0, n_scc, node_scc, scc_table, scc, scc0, cyclic0);
            if (level == 1) hipLaunchKernelGGL(po::k_cy_uncertain, dim3(R.rank_grid), dim3(256), 0, st, n0, n_scc, node_scc, scc_table, scc0, uncertain);
            PO_TRY(counters_home());
            const uint64_t singles = h->pinned[16 + po::PC_SINGLE];
            if (singles > n_scc || n_scc > n_flat) return fail(h, PO_ERR_HIP, std::string("internal: the SCCs of ") + name + " do not add up");
            const uint32_t n_cyclic = n_scc - (uint32_t)singles;
            if (!n_cyclic) break;
            if (n_cyclic > n0 - n_split) return fail(h, PO_ERR_HIP, std::string("internal: ") + name + " found more SCCs than unsplit nodes");
            for (uint32_t* p : {best_in, best_out, best_low}) HIP_TRY(h, hipMemsetAsync(p, 0xFF, (size_t)n_scc * 4, st));
            hipLaunchKernelGGL(po::k_cy_choose, dim3(R.rank_grid), dim3(256), 0, st, n0, n_scc, node_scc, scc_table, pflags, best_in, best_out,
                               best_low);
            hipLaunchKernelGGL(po::k_cy_apply, dim3(stride_grid(h, n_scc)), dim3(256), 0, st, n0, n_scc, scc_table, best_in, best_out, best_low,
                               level == 0 ? root_of : (const uint32_t*)nullptr, level == 0 && run == 0 ? rootless : (uint8_t*)nullptr, split, cnt);
            HIP_TRY(h, hipGetLastError());
            n_split += n_cyclic;
            S.n_split_levels = std::max(S.n_split_levels, level + 1);
        }
        S.n_split = std::max<uint64_t>(S.n_split, n_split);
        if (C[po::YC_BAD]) return fail(h, PO_ERR_HIP, std::string("internal: ") + name + " found no root for an SCC");
        if (run == 0) S.n_rootless = C[po::YC_ROOTLESS];
        // the stage of po_layout_superbubbles on the flat graph; the two drops of the lemma seed its discards
        const uint32_t n_flat = n0 + n_split;
        F.ev = ev;
        HIP_TRY(h, hipEventRecord(ev[3], st));
        SbWork W;
        const po_status staged = superbubble_dag(h, name, F, n_scc, W, [&] {
            if (n) hipLaunchKernelGGL(po::k_cy_seed_edges, dim3(R.edge_grid), dim3(256), 0, st, R.ends, n, n0, n_flat, exit_of, orig, filtered);
            hipLaunchKernelGGL(po::k_cy_seed_ranks, dim3(R.rank_grid), dim3(256), 0, st, n0, n_flat, exit_of, orig, filtered, dead, m_filtered);
            return true;
        });
        S.n_batches += W.n_batches;
        PO_TRY(staged);
        hipLaunchKernelGGL(po::k_cy_merge, dim3(R.rank_grid), dim3(256), 0, st, n0, n_flat, orig, F.root, exit_of, inside, total, m_exit, m_inside,
                           m_size, m_total, m_is_exit);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipEventRecord(ev[8], st));
        ++S.n_root_runs;
        // which rootless SCCs this run's root certified; the others go on along their cycle
        const bool more = S.n_rootless && (run == 0 || !open_sccs.empty());
        if (more)
            PO_TRY(land_outputs(h, {{uncertain, n0, bytes_a.data()}, {rootless, run == 0 ? n0 : 0u, bytes_b.data()}}, cnt, po::YC_N));
        else
            HIP_TRY(h, hipStreamSynchronize(st));
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev[7], ev[3]) == hipSuccess) ms_split += ms;
        if (hipEventElapsedTime(&ms, ev[3], ev[6]) == hipSuccess) ms_bubbles += ms;
        if (hipEventElapsedTime(&ms, ev[6], ev[8]) == hipSuccess) ms_merge += ms;
        if (!more) break;
        if (run == 0) {
            uint64_t seen = 0;
            for (uint32_t r = 0; r < n0; ++r) {
                if (!bytes_b[r]) continue;
                ++seen;
                if (bytes_a[r]) open_sccs.push_back(Rootless{r, {}, false});
                else ++S.n_certified;
            }
            if (seen != S.n_rootless) return fail(h, PO_ERR_HIP, std::string("internal: the rootless SCCs of ") + name + " do not add up");
            if (open_sccs.empty()) break;
            // one shortest cycle through the root of each: distances in rounds, the lowest-ranked parents, the walk back
            hipLaunchKernelGGL(po::k_cy_bfs_init, dim3(R.rank_grid), dim3(256), 0, st, n0, rootless, uncertain, is_root, dist, par, din, pin);
            RoundOps ops{h, st, R.rcnt};
            uint32_t rounds = 0;
            uint64_t ignored = 0;
            const int how = po::round_phase(ops, n0, [&](uint32_t j) {
                if (n) hipLaunchKernelGGL(po::k_cy_bfs_round, dim3(R.edge_grid), dim3(256), 0, st, R.ends, n, n0, is_root, dist, din, R.rcnt + j);
            }, rounds, S.n_batches, ignored);
            if (how == po::ROUNDS_FAILED) HIP_TRY(h, ops.err != hipSuccess ? ops.err : hipErrorUnknown);
            if (how != po::ROUNDS_DONE) return fail(h, PO_ERR_HIP, std::string("internal: the cycle search of ") + name + " reached its bound of n_order + 2 rounds");
            if (n) hipLaunchKernelGGL(po::k_cy_bfs_parents, dim3(R.edge_grid), dim3(256), 0, st, R.ends, n, n0, is_root, dist, din, par, pin);
            std::vector<uint32_t> h_par(n0), h_din(n0), h_pin(n0);
            PO_TRY(land_outputs(h, {{par, (size_t)n0 * 4, h_par.data()}, {din, (size_t)n0 * 4, h_din.data()}, {pin, (size_t)n0 * 4, h_pin.data()}},
                                cnt, po::YC_N));
            for (Rootless& x : open_sccs) {
                const uint32_t len = h_din[x.low];
                uint32_t v = h_pin[x.low];
                bool ok = len >= 1 && len <= n0;
                for (uint32_t i = 1; ok && i < len; ++i) {
                    ok = v < n0 && v != x.low;
                    if (ok) {
                        x.cycle.push_back(v);
                        v = h_par[v];
                    }
                }
                if (!ok || v != x.low) return fail(h, PO_ERR_HIP, std::string("internal: the cycle walk of ") + name + " does not close");
                std::reverse(x.cycle.begin(), x.cycle.end());
            }
        } else {
            for (Rootless& x : open_sccs)
                if (!x.done && !bytes_a[x.low]) {
                    x.done = true;
                    ++S.n_certified;
                }
        }
        bool any = false;
        for (Rootless& x : open_sccs) {
            if (x.done) continue;
            if (run >= x.cycle.size()) {   // the end of the cycle
                x.done = true;
                continue;
            }
            roots[x.low] = x.cycle[run];
            any = true;
        }
        if (!any) break;
    }
    // the outputs by rank, the table in entrance-rank order
    hipLaunchKernelGGL(po::k_cy_final, dim3(R.rank_grid), dim3(256), 0, st, n0, R.val, m_exit, m_inside, m_is_exit, loop, m_filtered, cyclic0,
                       m_root, U[UB_EXITOUT].as<uint32_t>(), U[UB_INSIDEOUT].as<uint32_t>(), U[UB_FLAGSOUT].as<uint8_t>(), cnt);
    HIP_TRY(h, hipGetLastError());
    PO_TRY(prefix_sum<uint8_t>(h, m_root, n0, R.index, &h->pinned[2]));
    HIP_TRY(h, hipStreamSynchronize(st));
    const uint64_t n64 = h->pinned[2];
    if (n64 > n0) return fail(h, PO_ERR_HIP, std::string("internal: the bubbles of ") + name + " do not add up");
    const uint32_t n_bubbles = (uint32_t)n64;
    if (n_bubbles)
        hipLaunchKernelGGL(po::k_sb_table, dim3(R.rank_grid), dim3(256), 0, st, n0, n_bubbles, R.val, m_root, R.index, m_exit, m_inside, m_total,
                           U[UB_TABLE].as<po::Bubble>());
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(ev[9], st));
    S.n_bubbles = n_bubbles;
    S.ms_split = ms_split;
    S.ms_bubbles = ms_bubbles;
    S.ms_merge = ms_merge;
    return PO_OK;
}

// the stage's counters, once a synchronise has brought the YC_N words of YB_CNT to words 16.. of the landing zone
po_status superbubble_all_counts(po_handle* h, const char* const name, po_superbubble_all_stats& S) {
    S.n_nested = h->pinned[16 + po::YC_NESTED];
    S.n_cyclic_bubbles = h->pinned[16 + po::YC_CYCLIC];
    S.n_edge_filtered = h->pinned[16 + po::YC_FILTERED];
    if (S.n_nested > S.n_bubbles || S.n_cyclic_bubbles > S.n_bubbles)
        return fail(h, PO_ERR_HIP, std::string("internal: the counts of ") + name + " do not add up");
    return PO_OK;
}

po_status run_superbubbles_all(po_handle* h, po_result* graph, uint32_t* exit_out, uint32_t* inside_out, uint8_t* flags_out,
                               po_superbubble* table_out, uint64_t* n_bubbles_out) {
    const char* const name = "po_layout_superbubbles_all";
    po_superbubble_all_stats& S = h->sastats;
    S = po_superbubble_all_stats();
    DevBuf* U = h->d_sb;
    RankedGraph R;
    PO_TRY(superbubble_all_stage(h, graph, name, EV_CYCLIC, S, [](size_t, size_t) { return PO_OK; }, R, S));
    if (!R.ev || !R.n_order) return PO_OK;
    const uint32_t n0 = R.n_order, n_bubbles = (uint32_t)S.n_bubbles;
    hipEvent_t* ev = R.ev;
    PO_TRY(land_outputs(h, {{U[UB_TABLE].p, (size_t)n_bubbles * sizeof(po_superbubble), table_out},
                            {U[UB_EXITOUT].p, (size_t)n0 * 4, exit_out}, {U[UB_INSIDEOUT].p, (size_t)n0 * 4, inside_out},
                            {U[UB_FLAGSOUT].p, n0, flags_out}}, h->d_cy[YB_CNT].as<unsigned long long>(), po::YC_N));
    PO_TRY(superbubble_all_counts(h, name, S));
    *n_bubbles_out = n_bubbles;
    (void)hipEventElapsedTime(&S.ms_ranks, ev[0], ev[1]);
    (void)hipEventElapsedTime(&S.ms_total, ev[0], ev[9]);
    return PO_OK;
}

// ---- the bubble chains (po_layout_bubblechains, bubblechains.hip.h) -------------------------------------------------------

// what the bubble-chain stage counts, for the stats of its callers
struct BcWork {
    uint64_t n_bubbles = 0, n_top = 0, n_chains = 0, n_short = 0, n_chain_nodes = 0, n_chain_edges = 0, n_ring_chains = 0, n_ring_bubbles = 0;
    uint32_t max_chain_bubbles = 0, n_nest_rounds = 0, n_chain_rounds = 0, n_batches = 0, n_ring_rounds = 0;
    int ev_last = 6;   // the last event of the bubble source: the stage records the two behind it
};

// What a bubble source leaves for the bubble-chain stage, per rank of the graph: the byte "enters a surviving bubble",
// exit_of, the holder, and the counts.  `rings`: bubbles may lie inside an SCC, so their links may close to rings.
struct BubbleSource {
    const uint8_t* enters = nullptr;
    const uint32_t *exit_of = nullptr, *inside = nullptr;
    uint64_t n_bubbles = 0, n_nested = 0;
    uint32_t n_batches = 0;
    int ev_last = 6;
    bool rings = false;
};

// the superbubbles of the acyclic partitions: superbubble_stage, as po_layout_bubblechains, po_layout_contigs and
// po_phase_paths take them
struct AcyclicBubbles {
    template <class Stats, class Own>
    po_status operator()(po_handle* h, po_result* graph, const char* const name, int ev_first, Stats& stats, Own&& own, RankedGraph& R,
                         BubbleSource& src) const {
        SbWork W;
        const po_status staged = superbubble_stage(h, graph, name, ev_first, stats, own, R, W);
        src.n_bubbles = W.n_bubbles;
        src.n_nested = W.n_nested;
        src.n_batches = W.n_batches;
        PO_TRY(staged);
        src.enters = R.root;
        src.exit_of = h->d_sb[UB_EXIT].as<uint32_t>();
        src.inside = h->d_sb[UB_INSIDE].as<uint32_t>();
        return PO_OK;
    }
};

// the superbubbles of the whole graph: superbubble_all_stage, its counters brought home (one synchronise more), as
// po_layout_bubblechains_all and po_layout_contigs_all take them.  A holds the first stage's stats.
struct CyclicBubbles {
    po_superbubble_all_stats& A;
    template <class Stats, class Own>
    po_status operator()(po_handle* h, po_result* graph, const char* const name, int ev_first, Stats& stats, Own&& own, RankedGraph& R,
                         BubbleSource& src) const {
        src.ev_last = 9;
        const po_status staged = superbubble_all_stage(h, graph, name, ev_first, stats, own, R, A);
        src.n_batches = A.n_batches;
        PO_TRY(staged);
        if (!R.ev || !R.n_order) return PO_OK;
        HIP_TRY(h, hipMemcpyAsync(h->pinned + 16, h->d_cy[YB_CNT].p, po::YC_N * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        PO_TRY(superbubble_all_counts(h, name, A));
        src.n_bubbles = A.n_bubbles;
        src.n_nested = A.n_nested;
        src.rings = A.n_cyclic_bubbles > 0;   // (rings exist only inside SCCs)
        src.enters = h->d_cy[YB_MROOT].as<uint8_t>();
        src.exit_of = h->d_cy[YB_MEXIT].as<uint32_t>();
        src.inside = h->d_cy[YB_MINSIDE].as<uint32_t>();
        return PO_OK;
    }
};

// The bubble-chain stage on the device, as po_layout_bubblechains and po_layout_contigs run it (`name`, the first of the
// caller's events, the caller's stats for ranked_open): the bubble source -- AcyclicBubbles, or CyclicBubbles for the calls
// that end in _all -- with the workspaces of d_bc and the caller's `own`, then everything up to the table and the three
// arrays, all left in d_bc -- the chain per rank in HB_CHAINOUT; the counters in HB_CNT.  Records the two events behind the
// source's last (ev[7] and ev[8] behind AcyclicBubbles).  Where the source says that links may close to rings, the election
// of ringchains.hip.h runs between the heads and the ranking.  S is filled whatever the outcome.  !R.ev or !R.n_order:
// nothing to do.
template <class Stats, class Own, class Source = AcyclicBubbles>
po_status bubblechain_stage(po_handle* h, po_result* graph, const char* const name, int ev_first, Stats& stats, uint32_t min_nodes, Own&& own,
                            RankedGraph& R, BcWork& S, Source&& source = Source()) {
    hipStream_t st = h->stream;
    DevBuf* B = h->d_bc;
    BubbleSource W;
    const po_status staged = source(h, graph, name, ev_first, stats, [&](size_t nn, size_t ne) {
        PO_TRY(ensure(h, B[HB_CNT], 128));
        for (int k : {HB_FW, HB_NEXT, HB_PRED, HB_TOP, HB_JB0, HB_JB1, HB_HOPS0, HB_HOPS1, HB_NHEAD, HB_NPOS, HB_CB, HB_CN, HB_LAST, HB_CHAINOUT,
                      HB_BUBBLEOUT})
            PO_TRY(ensure(h, B[k], nn * 4));
        PO_TRY(ensure(h, B[HB_CE], nn * 8));
        PO_TRY(ensure(h, B[HB_EDGEOUT], ne * 4));
        PO_TRY(ensure(h, B[HB_TABLE], nn * sizeof(po::BubbleChain)));
        if (!std::is_same<typename std::decay<Source>::type, AcyclicBubbles>::value)
            for (int k : {HB_RPTR0, HB_RPTR1, HB_RMN0, HB_RMN1}) PO_TRY(ensure(h, B[k], nn * 4));
        return own(nn, ne);
    }, R, W);
    S.n_bubbles = W.n_bubbles;
    S.n_batches = W.n_batches;
    S.ev_last = W.ev_last;
    PO_TRY(staged);
    if (!R.ev || !R.n_order) return PO_OK;
    const uint32_t n = R.n, n_order = R.n_order;
    hipEvent_t* ev = R.ev;
    unsigned long long *cnt = B[HB_CNT].as<unsigned long long>(), *ce = B[HB_CE].as<unsigned long long>();
    uint32_t *fw = B[HB_FW].as<uint32_t>(), *next = B[HB_NEXT].as<uint32_t>(), *pred = B[HB_PRED].as<uint32_t>(), *top = B[HB_TOP].as<uint32_t>(),
             *jb[2] = {B[HB_JB0].as<uint32_t>(), B[HB_JB1].as<uint32_t>()}, *hops[2] = {B[HB_HOPS0].as<uint32_t>(), B[HB_HOPS1].as<uint32_t>()},
             *nhead = B[HB_NHEAD].as<uint32_t>(), *npos = B[HB_NPOS].as<uint32_t>(), *cb = B[HB_CB].as<uint32_t>(), *cn = B[HB_CN].as<uint32_t>(),
             *last = B[HB_LAST].as<uint32_t>(), *d_chain = B[HB_CHAINOUT].as<uint32_t>(), *d_bubble = B[HB_BUBBLEOUT].as<uint32_t>(),
             *d_edge = B[HB_EDGEOUT].as<uint32_t>();
    po::BubbleChain* table = B[HB_TABLE].as<po::BubbleChain>();
    const uint32_t *exit_of = W.exit_of, *inside = W.inside;
    const int n_counters = W.rings ? (int)po::HKR_N : (int)po::HK_N;
    volatile uint64_t* C = h->pinned + 48;   // this stage's counters on the host (words 16.. and 32.. are the scaffold's)
    auto counters_home = [&]() -> po_status {
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(h->pinned + 48, cnt, (size_t)n_counters * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipStreamSynchronize(st));
        return PO_OK;
    };
    // top-level entrances (the source's byte "enters a surviving bubble"; R.root itself behind AcyclicBubbles), their links,
    // the heads
    HIP_TRY(h, hipMemsetAsync(cnt, 0, 128, st));
    hipLaunchKernelGGL(po::k_bc_init, dim3(R.rank_grid), dim3(256), 0, st, n_order, W.enters, inside, fw, next, pred, top, cb, cn, ce, last);
    hipLaunchKernelGGL(po::k_bc_link, dim3(R.rank_grid), dim3(256), 0, st, n_order, fw, exit_of, next, pred, cnt);
    hipLaunchKernelGGL(po::k_bc_heads, dim3(R.rank_grid), dim3(256), 0, st, n_order, pred, fw, jb[0], hops[0], cnt);
    PO_TRY(counters_home());
    const uint64_t n_top = C[po::HK_TOP];
    uint64_t n_heads = C[po::HK_HEADS];
    if (n_top + W.n_nested != W.n_bubbles || n_heads > n_top || (n_top && !n_heads && !W.rings))
        return fail(h, PO_ERR_HIP, std::string("internal: the top-level bubbles of ") + name + " do not add up");
    S.n_top = n_top;
    // one leader per ring of links: a fixed number of doubling rounds between two buffer pairs, nothing read back between them
    if (n_top && W.rings) {
        uint32_t *ptr[2] = {B[HB_RPTR0].as<uint32_t>(), B[HB_RPTR1].as<uint32_t>()}, *mn[2] = {B[HB_RMN0].as<uint32_t>(), B[HB_RMN1].as<uint32_t>()};
        const uint32_t rounds = po::ring_rounds(n_top);
        hipLaunchKernelGGL(po::k_rc_init, dim3(R.rank_grid), dim3(256), 0, st, n_order, jb[0], ptr[0], mn[0]);
        for (uint32_t k = 0; k < rounds; ++k)
            hipLaunchKernelGGL(po::k_rc_round, dim3(R.rank_grid), dim3(256), 0, st, n_order, ptr[k & 1], mn[k & 1], ptr[(k & 1) ^ 1], mn[(k & 1) ^ 1]);
        hipLaunchKernelGGL(po::k_rc_leaders, dim3(R.rank_grid), dim3(256), 0, st, n_order, ptr[rounds & 1], mn[rounds & 1], fw, jb[0], hops[0], cnt);
        PO_TRY(counters_home());
        S.n_ring_rounds = rounds;
        S.n_ring_chains = C[po::HKR_RINGS];
        if (C[po::HK_HEADS] != n_heads + S.n_ring_chains || C[po::HK_HEADS] > n_top || !C[po::HK_HEADS])
            return fail(h, PO_ERR_HIP, std::string("internal: the heads and ring leaders of ") + name + " do not add up");
        n_heads = C[po::HK_HEADS];
    }
    RoundOps ops{h, st, R.rcnt};
    uint64_t ignored = 0;
    // the outermost holder of every rank inside a bubble: needed only where a bubble lies inside another
    if (n_top && W.n_nested) {
        const int how = po::round_phase(ops, W.n_nested, [&](uint32_t j) {
            hipLaunchKernelGGL(po::k_bc_nest, dim3(R.rank_grid), dim3(256), 0, st, n_order, top, R.rcnt + j);
        }, S.n_nest_rounds, S.n_batches, ignored);
        if (how == po::ROUNDS_FAILED) HIP_TRY(h, ops.err != hipSuccess ? ops.err : hipErrorUnknown);
        if (how != po::ROUNDS_DONE) return fail(h, PO_ERR_HIP, std::string("internal: the holders of ") + name + " reached their bound of nested + 2 rounds");
    }
    // list ranking of the top-level entrances toward their head: ping-pong, the last launch wrote jb[fin] / hops[fin]
    uint32_t launched = 0;
    if (n_top) {
        const int how = po::round_phase(ops, n_top, [&](uint32_t j) {
            const uint32_t a = launched & 1, b = a ^ 1;
            hipLaunchKernelGGL(po::k_bc_jump, dim3(R.rank_grid), dim3(256), 0, st, n_order, jb[a], hops[a], jb[b], hops[b], R.rcnt + j);
            ++launched;
        }, S.n_chain_rounds, S.n_batches, ignored);
        if (how == po::ROUNDS_FAILED) HIP_TRY(h, ops.err != hipSuccess ? ops.err : hipErrorUnknown);
        if (how != po::ROUNDS_DONE) return fail(h, PO_ERR_HIP, std::string("internal: the ranking of ") + name + " reached its bound of top-level + 2 rounds");
    }
    const uint32_t fin = launched & 1;
    HIP_TRY(h, hipEventRecord(ev[W.ev_last + 1], st));
    // chain and position of every rank, the sums per head, the filter, the numbering of the surviving heads
    hipLaunchKernelGGL(po::k_bc_place, dim3(R.rank_grid), dim3(256), 0, st, n_order, fw, next, pred, top, exit_of, jb[fin], hops[fin], nhead, npos,
                       cb, cn, last, cnt);
    if (S.n_ring_chains) hipLaunchKernelGGL(po::k_rc_close, dim3(R.rank_grid), dim3(256), 0, st, n_order, fw, cb, last, cnt);
    if (n) hipLaunchKernelGGL(po::k_bc_edges, dim3(R.edge_grid), dim3(256), 0, st, R.ends, n, n_order, nhead, ce);
    hipLaunchKernelGGL(po::k_bc_filter, dim3(R.rank_grid), dim3(256), 0, st, n_order, min_nodes, fw, cb, cn, ce, R.root, cnt);
    HIP_TRY(h, hipGetLastError());
    PO_TRY(prefix_sum<uint8_t>(h, R.root, n_order, R.index, &h->pinned[2]));
    PO_TRY(counters_home());
    if (C[po::HK_BAD]) return fail(h, PO_ERR_HIP, std::string("internal: a node of ") + name + " reached no head");
    const uint64_t n64 = h->pinned[2];
    if (n64 != C[po::HK_CHAINS] || n64 + C[po::HK_SHORT] != n_heads || C[po::HK_CNODES] > n_order || C[po::HK_CEDGES] > n ||
        C[po::HK_MAXB] > n_top)
        return fail(h, PO_ERR_HIP, std::string("internal: the chains of ") + name + " do not add up");
    const uint32_t n_chains = (uint32_t)n64;
    S.n_chains = n_chains;
    S.n_short = C[po::HK_SHORT];
    S.n_chain_nodes = C[po::HK_CNODES];
    S.n_chain_edges = C[po::HK_CEDGES];
    S.max_chain_bubbles = (uint32_t)C[po::HK_MAXB];
    if (S.n_ring_chains) {
        S.n_ring_bubbles = C[po::HKR_RBUBBLES];
        if (S.n_ring_bubbles < S.n_ring_chains || S.n_ring_bubbles > n_top)
            return fail(h, PO_ERR_HIP, std::string("internal: the ring chains of ") + name + " do not add up");
    }
    if (n_chains)
        hipLaunchKernelGGL(po::k_bc_table, dim3(R.rank_grid), dim3(256), 0, st, n_order, n_chains, R.val, R.root, R.index, last, cb, cn, ce, table);
    hipLaunchKernelGGL(po::k_bc_nodes, dim3(R.rank_grid), dim3(256), 0, st, n_order, n_chains, R.root, R.index, nhead, npos, d_chain, d_bubble);
    if (n) hipLaunchKernelGGL(po::k_bc_edge_out, dim3(R.edge_grid), dim3(256), 0, st, R.ends, n, n_order, d_chain, d_edge);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(ev[W.ev_last + 2], st));
    return PO_OK;
}

po_status run_bubblechains(po_handle* h, po_result* graph, uint32_t min_nodes, uint32_t* chain_out, uint32_t* bubble_out,
                           uint32_t* edge_out, po_bubblechain* table_out, uint64_t* n_chains_out) {
    po_bubblechain_stats& S = h->bcstats;
    S = po_bubblechain_stats();
    DevBuf* B = h->d_bc;
    RankedGraph R;
    BcWork W;
    const po_status staged = bubblechain_stage(h, graph, "po_layout_bubblechains", EV_BUBBLECHAINS, S, min_nodes,
                                               [](size_t, size_t) { return PO_OK; }, R, W);
    S.n_bubbles = W.n_bubbles;
    S.n_top = W.n_top;
    S.n_chains = W.n_chains;
    S.n_short = W.n_short;
    S.n_chain_nodes = W.n_chain_nodes;
    S.n_chain_edges = W.n_chain_edges;
    S.max_chain_bubbles = W.max_chain_bubbles;
    S.n_nest_rounds = W.n_nest_rounds;
    S.n_chain_rounds = W.n_chain_rounds;
    S.n_batches = W.n_batches;
    PO_TRY(staged);
    if (!R.ev || !R.n_order) return PO_OK;
    const uint32_t n = R.n, n_order = R.n_order, n_chains = (uint32_t)W.n_chains;
    hipEvent_t* ev = R.ev;
    static_assert(sizeof(po_bubblechain) == sizeof(po::BubbleChain) && sizeof(po_bubblechain) == 24, "po_bubblechain is the device's table entry");
    PO_TRY(land_outputs(h, {{B[HB_TABLE].p, (size_t)n_chains * sizeof(po_bubblechain), table_out},
                            {B[HB_CHAINOUT].p, (size_t)n_order * 4, chain_out}, {B[HB_BUBBLEOUT].p, (size_t)n_order * 4, bubble_out},
                            {B[HB_EDGEOUT].p, (size_t)n * 4, edge_out}}, B[HB_CNT].as<unsigned long long>(), po::HK_N));
    *n_chains_out = n_chains;
    (void)hipEventElapsedTime(&S.ms_superbubbles, ev[0], ev[6]);
    (void)hipEventElapsedTime(&S.ms_chains, ev[6], ev[7]);
    (void)hipEventElapsedTime(&S.ms_label, ev[7], ev[8]);
    (void)hipEventElapsedTime(&S.ms_total, ev[0], ev[8]);
    return PO_OK;
}

// The same behind the superbubbles of the whole graph (CyclicBubbles): a chain may be a ring, its head the lowest-ranked
// entrance and its last exit that head again.
po_status run_bubblechains_all(po_handle* h, po_result* graph, uint32_t min_nodes, uint32_t* chain_out, uint32_t* bubble_out,
                               uint32_t* edge_out, po_bubblechain* table_out, uint64_t* n_chains_out) {
    po_bubblechain_all_stats& S = h->bcastats;
    S = po_bubblechain_all_stats();
    DevBuf* B = h->d_bc;
    RankedGraph R;
    BcWork W;
    po_superbubble_all_stats A = {};
    const po_status staged = bubblechain_stage(h, graph, "po_layout_bubblechains_all", EV_CHAINS_ALL, S, min_nodes,
                                               [](size_t, size_t) { return PO_OK; }, R, W, CyclicBubbles{A});
    S.n_bubbles = W.n_bubbles;
    S.n_top = W.n_top;
    S.n_chains = W.n_chains;
    S.n_short = W.n_short;
    S.n_chain_nodes = W.n_chain_nodes;
    S.n_chain_edges = W.n_chain_edges;
    S.n_ring_chains = W.n_ring_chains;
    S.n_ring_bubbles = W.n_ring_bubbles;
    S.n_cyclic_bubbles = A.n_cyclic_bubbles;
    S.max_chain_bubbles = W.max_chain_bubbles;
    S.n_nest_rounds = W.n_nest_rounds;
    S.n_chain_rounds = W.n_chain_rounds;
    S.n_batches = W.n_batches;
    S.n_ring_rounds = W.n_ring_rounds;
    S.n_root_runs = A.n_root_runs;
    S.n_split_levels = A.n_split_levels;
    PO_TRY(staged);
    if (!R.ev || !R.n_order) return PO_OK;
    const uint32_t n = R.n, n_order = R.n_order, n_chains = (uint32_t)W.n_chains;
    hipEvent_t* ev = R.ev;
    const int e = W.ev_last;
    PO_TRY(land_outputs(h, {{B[HB_TABLE].p, (size_t)n_chains * sizeof(po_bubblechain), table_out},
                            {B[HB_CHAINOUT].p, (size_t)n_order * 4, chain_out}, {B[HB_BUBBLEOUT].p, (size_t)n_order * 4, bubble_out},
                            {B[HB_EDGEOUT].p, (size_t)n * 4, edge_out}}, B[HB_CNT].as<unsigned long long>(), po::HKR_N));
    *n_chains_out = n_chains;
    (void)hipEventElapsedTime(&S.ms_superbubbles, ev[0], ev[e]);
    (void)hipEventElapsedTime(&S.ms_chains, ev[e], ev[e + 1]);
    (void)hipEventElapsedTime(&S.ms_label, ev[e + 1], ev[e + 2]);
    (void)hipEventElapsedTime(&S.ms_total, ev[0], ev[e + 2]);
    return PO_OK;
}

// ---- paths, interior and exit predecessors of every top-level bubble (po_phase_paths, paths.hip.h) ---------------------------

constexpr uint64_t PATHS_MAX_LISTED = 1ull << 30;   // listed paths of one call (each has two nodes at the least)
constexpr uint64_t PATHS_MAX_NODES = 1ull << 31;    // their nodes together

po_status run_paths(po_handle* h, po_result* graph, uint64_t max_paths, po_result* r) {
    const char* const name = "po_phase_paths";
    hipStream_t st = h->stream;
    po_paths_stats& S = h->ppstats;
    S = po_paths_stats();
    r->special = 4;
    r->elem = 1;
    r->pp = po_paths_dims();
    DevBuf* B = h->d_pp;
    DevBuf* O = r->d_pp;
    RankedGraph R;
    BcWork W;
    uint32_t pad_e = 1;
    const po_status staged = bubblechain_stage(h, graph, name, EV_PATHS, S, 1u, [&](size_t nn, size_t ne) {
        pad_e = po::merge_sort_pad((uint32_t)ne);
        PO_TRY(ensure(h, B[QB_CNT], 128));
        for (int k : {QB_NB, QB_COFF, QB_HOME, QB_BIDX, QB_BENT, QB_DONE, QB_OFIRST, QB_OLAST, QB_IFIRST, QB_ILAST, QB_NLIST, QB_NPRED, QB_NIN})
            PO_TRY(ensure(h, B[k], nn * 4));
        PO_TRY(ensure(h, B[QB_COUNT], nn * 8));
        for (int k : {QB_KEYOUT, QB_KEYIN}) PO_TRY(ensure(h, B[k], (size_t)pad_e * 8));
        return PO_OK;
    }, R, W);
    S.n_batches = W.n_batches;
    PO_TRY(staged);
    if (!R.ev || !R.n_order || !W.n_top) return PO_OK;   // (no bubble: every size 0)
    const uint32_t n = R.n, n_order = R.n_order, n_chains = (uint32_t)W.n_chains, n_b = (uint32_t)W.n_top;
    if (!n) return fail(h, PO_ERR_HIP, std::string("internal: ") + name + " found bubbles in a graph without edges");
    hipEvent_t* ev = R.ev;
    unsigned long long *cnt = B[QB_CNT].as<unsigned long long>(), *count = B[QB_COUNT].as<unsigned long long>(),
                       *key_out = B[QB_KEYOUT].as<unsigned long long>(), *key_in = B[QB_KEYIN].as<unsigned long long>(),
                       *key_inside = h->d_rank[RK_KEY].as<unsigned long long>();   // (the rank sort is over: pad(n_total) words)
    uint32_t *nb = B[QB_NB].as<uint32_t>(), *coff = B[QB_COFF].as<uint32_t>(), *home = B[QB_HOME].as<uint32_t>(),
             *bidx = B[QB_BIDX].as<uint32_t>(), *bent = B[QB_BENT].as<uint32_t>(), *done = B[QB_DONE].as<uint32_t>(),
             *ofirst = B[QB_OFIRST].as<uint32_t>(), *olast = B[QB_OLAST].as<uint32_t>(), *ifirst = B[QB_IFIRST].as<uint32_t>(),
             *ilast = B[QB_ILAST].as<uint32_t>(), *n_list = B[QB_NLIST].as<uint32_t>(), *n_pred = B[QB_NPRED].as<uint32_t>(),
             *n_in = B[QB_NIN].as<uint32_t>();
    const uint32_t *fw = h->d_bc[HB_FW].as<uint32_t>(), *top = h->d_bc[HB_TOP].as<uint32_t>(), *pred = h->d_bc[HB_PRED].as<uint32_t>(),
                   *chain = h->d_bc[HB_CHAINOUT].as<uint32_t>(), *pos = h->d_bc[HB_BUBBLEOUT].as<uint32_t>(),
                   *exit_of = h->d_sb[UB_EXIT].as<uint32_t>(), *total = h->d_sb[UB_TOTAL].as<uint32_t>();
    const po::BubbleChain* chains = h->d_bc[HB_TABLE].as<po::BubbleChain>();
    const uint32_t pad_n = po::merge_sort_pad(n);   // (<= pad_e)
    const uint32_t bubble_grid = stride_grid(h, (uint64_t)n_b + 1);
    volatile uint64_t* C = h->pinned + 48;   // this stage's counters on the host (words 16.. and 32.. are the scaffold's)
    auto counters_home = [&]() -> po_status {
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(h->pinned + 48, cnt, po::QK_N * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipStreamSynchronize(st));
        return PO_OK;
    };
    auto sort_keys = [&](unsigned long long* key, uint32_t count_, uint32_t pad) {
        po::merge_sort_steps(count_, [&](uint32_t j, uint32_t k) {
            hipLaunchKernelGGL(po::k_pp_bitonic, dim3(stride_grid(h, pad)), dim3(256), 0, st, key, pad, j, k);
        });
    };
    static_assert(sizeof(po_bubble_paths) == sizeof(po::BubblePaths) && sizeof(po_bubble_paths) == 40, "po_bubble_paths is the device's table entry");
    // the result's table and its three offset arrays: sized by the bubbles
    PO_TRY(ensure(h, O[PR_TABLE], (size_t)n_b * sizeof(po::BubblePaths), 1.0, false));
    for (int k : {PR_INOFF, PR_PREDOFF, PR_BPO}) PO_TRY(ensure(h, O[k], ((size_t)n_b + 1) * 4, 1.0, false));
    po::BubblePaths* table = O[PR_TABLE].as<po::BubblePaths>();
    uint32_t *in_off = O[PR_INOFF].as<uint32_t>(), *pred_off = O[PR_PREDOFF].as<uint32_t>(), *bpo = O[PR_BPO].as<uint32_t>();
    // the bubbles numbered by (chain, position); home of every rank; the edges by tail and, into exits, by head
    HIP_TRY(h, hipMemsetAsync(cnt, 0, 128, st));
    hipLaunchKernelGGL(po::k_pp_chain_counts, dim3(stride_grid(h, (uint64_t)n_chains + 1)), dim3(256), 0, st, n_chains, chains, nb);
    HIP_TRY(h, hipGetLastError());
    PO_TRY(prefix_sum<uint32_t>(h, nb, (uint64_t)n_chains + 1, coff, &h->pinned[2]));
    HIP_TRY(h, hipMemsetAsync(bent, 0xFF, (size_t)n_order * 4, st));
    for (uint32_t* p : {ofirst, olast, ifirst, ilast}) HIP_TRY(h, hipMemsetAsync(p, 0, (size_t)n_order * 4, st));
    hipLaunchKernelGGL(po::k_pp_bubbles, dim3(R.rank_grid), dim3(256), 0, st, n_order, n_chains, n_b, fw, top, chain, pos, coff, total, home, bidx,
                       bent, done, count, cnt);
    hipLaunchKernelGGL(po::k_pp_keys, dim3(stride_grid(h, pad_n)), dim3(256), 0, st, R.ends, n, n_order, pad_n, home, exit_of, pred, key_out, key_in,
                       cnt);
    sort_keys(key_out, n, pad_n);
    sort_keys(key_in, n, pad_n);
    hipLaunchKernelGGL(po::k_pp_segments, dim3(R.edge_grid), dim3(256), 0, st, key_out, n, n_order, ofirst, olast);
    hipLaunchKernelGGL(po::k_pp_segments, dim3(R.edge_grid), dim3(256), 0, st, key_in, n, n_order, ifirst, ilast);
    PO_TRY(counters_home());
    if (h->pinned[2] != n_b || C[po::QK_BAD] || C[po::QK_MAXIN] > n_order)
        return fail(h, PO_ERR_HIP, std::string("internal: the bubbles of ") + name + " do not add up");
    S.n_bubbles = n_b;
    S.n_stray_edges = C[po::QK_STRAY];
    const uint64_t max_inside = C[po::QK_MAXIN];
    // the counts: a member sums its successors once an earlier launch has finished them all; bounded by round_phase
    {
        RoundOps ops{h, st, R.rcnt};
        uint64_t ignored = 0;
        uint32_t launch = 0;
        const int how = po::round_phase(ops, max_inside, [&](uint32_t j) {
            ++launch;
            hipLaunchKernelGGL(po::k_pp_count, dim3(R.rank_grid), dim3(256), 0, st, n_order, n, launch, home, exit_of, ofirst, olast, key_out, R.ends,
                               done, count, R.rcnt + j);
        }, S.n_count_rounds, S.n_batches, ignored);
        if (how == po::ROUNDS_FAILED) HIP_TRY(h, ops.err != hipSuccess ? ops.err : hipErrorUnknown);
        if (how != po::ROUNDS_DONE)
            return fail(h, PO_ERR_HIP, std::string("internal: the counts of ") + name + " reached their bound of the largest n_inside + 2 rounds");
    }
    HIP_TRY(h, hipEventRecord(ev[9], st));
    // the table; how many paths, predecessors and interior nodes every bubble adds, and where they go
    hipLaunchKernelGGL(po::k_pp_table, dim3(bubble_grid), dim3(256), 0, st, n_b, n_order, (unsigned long long)max_paths, bent, exit_of, R.val, chain,
                       pos, total, count, ifirst, ilast, table, n_list, n_pred, n_in, cnt);
    HIP_TRY(h, hipGetLastError());
    PO_TRY(prefix_sum<uint32_t>(h, n_list, (uint64_t)n_b + 1, bpo, &h->pinned[2]));
    PO_TRY(prefix_sum<uint32_t>(h, n_pred, (uint64_t)n_b + 1, pred_off, &h->pinned[3]));
    PO_TRY(prefix_sum<uint32_t>(h, n_in, (uint64_t)n_b + 1, in_off, &h->pinned[4]));
    PO_TRY(counters_home());
    S.n_bare = C[po::QK_BARE];
    S.n_unlisted = C[po::QK_UNLISTED];
    S.n_saturated = C[po::QK_SATURATED];
    S.max_paths_seen = C[po::QK_MAXPATHS];
    const uint64_t listed64 = C[po::QK_LISTED], preds64 = h->pinned[3], inside64 = h->pinned[4];
    // (decided from the counts alone, before anything is listed: the caller lowers max_paths)
    if (listed64 >= PATHS_MAX_LISTED)
        return fail(h, PO_ERR_CAPACITY, std::string(name) + ": at least " + std::to_string(listed64) + " paths to list in one call, at most 2^30 - 1");
    if (h->pinned[2] != listed64 || preds64 > n || inside64 > n_order)
        return fail(h, PO_ERR_HIP, std::string("internal: the offsets of ") + name + " do not add up");
    const uint32_t n_listed = (uint32_t)listed64, n_preds = (uint32_t)preds64, n_inside = (uint32_t)inside64;
    PO_TRY(ensure(h, B[QB_PLEN], ((size_t)n_listed + 1) * 4));
    PO_TRY(ensure(h, O[PR_POFF], ((size_t)n_listed + 1) * 4, 1.0, false));
    PO_TRY(ensure(h, O[PR_PREDNODE], std::max<size_t>((size_t)n_preds * 4, 256), 1.0, false));
    PO_TRY(ensure(h, O[PR_PREDW], std::max<size_t>((size_t)n_preds * 4, 256), 1.0, false));
    PO_TRY(ensure(h, O[PR_INNODES], std::max<size_t>((size_t)n_inside * 4, 256), 1.0, false));
    uint32_t *plen = B[QB_PLEN].as<uint32_t>(), *poff = O[PR_POFF].as<uint32_t>(), *pred_node = O[PR_PREDNODE].as<uint32_t>(),
             *inside_nodes = O[PR_INNODES].as<uint32_t>();
    int32_t* pred_weight = O[PR_PREDW].as<int32_t>();
    // the predecessors of the exits; the interior of every bubble by (bubble, rank)
    hipLaunchKernelGGL(po::k_pp_preds, dim3(R.edge_grid), dim3(256), 0, st, n, n_order, n_preds, key_in, R.ends, graph->d_rows.as<po::Edge>(), pred,
                       bidx, ifirst, pred_off, R.val, pred_node, pred_weight, cnt);
    const uint32_t pad_o = po::merge_sort_pad(n_order);   // (<= pad(n_total), what RK_KEY holds)
    hipLaunchKernelGGL(po::k_pp_inside_keys, dim3(stride_grid(h, pad_o)), dim3(256), 0, st, n_order, pad_o, home, bidx, key_inside, cnt);
    sort_keys(key_inside, n_order, pad_o);
    if (n_inside) hipLaunchKernelGGL(po::k_pp_inside, dim3(stride_grid(h, n_inside)), dim3(256), 0, st, n_inside, n_order, key_inside, R.val, inside_nodes);
    // the length of every listed path, their offsets, then the nodes
    const uint32_t path_grid = stride_grid(h, (uint64_t)n_listed + 1);
    hipLaunchKernelGGL(po::k_pp_walk<false>, dim3(path_grid), dim3(256), 0, st, n_listed, n_b, n_order, n, 0u, bpo, bent, exit_of, total, home, ofirst,
                       olast, key_out, R.ends, count, R.val, plen, (const uint32_t*)nullptr, (uint32_t*)nullptr, cnt);
    HIP_TRY(h, hipGetLastError());
    PO_TRY(prefix_sum<uint32_t>(h, plen, (uint64_t)n_listed + 1, poff, &h->pinned[5]));
    PO_TRY(counters_home());
    if (C[po::QK_BAD] || C[po::QK_INSIDE] != n_inside)
        return fail(h, PO_ERR_HIP, std::string("internal: the interior nodes or the predecessors of ") + name + " do not add up");
    if (C[po::QK_WALK]) return fail(h, PO_ERR_HIP, std::string("internal: a path of ") + name + " did not reach its exit within n_inside + 1 steps");
    const uint64_t nodes64 = h->pinned[5];
    if (nodes64 >= PATHS_MAX_NODES)
        return fail(h, PO_ERR_CAPACITY, std::string(name) + ": the listed paths hold " + std::to_string(nodes64) + " nodes together, at most 2^31 - 1");
    if (nodes64 < 2 * listed64 || C[po::QK_MAXLEN] > max_inside + 2)
        return fail(h, PO_ERR_HIP, std::string("internal: the path lengths of ") + name + " do not add up");
    const uint32_t n_path_nodes = (uint32_t)nodes64;
    PO_TRY(ensure(h, O[PR_PATHS], std::max<size_t>((size_t)n_path_nodes * 4, 256), 1.0, false));
    uint32_t* path_nodes = O[PR_PATHS].as<uint32_t>();
    if (n_listed)
        hipLaunchKernelGGL(po::k_pp_walk<true>, dim3(path_grid), dim3(256), 0, st, n_listed, n_b, n_order, n, n_path_nodes, bpo, bent, exit_of, total,
                           home, ofirst, olast, key_out, R.ends, count, R.val, (uint32_t*)nullptr, poff, path_nodes, cnt);
    hipLaunchKernelGGL(po::k_pp_bubble_nodes, dim3(stride_grid(h, n_b)), dim3(256), 0, st, n_b, bpo, poff, table);
    HIP_TRY(h, hipEventRecord(ev[10], st));
    PO_TRY(counters_home());
    if (C[po::QK_WALK]) return fail(h, PO_ERR_HIP, std::string("internal: a path of ") + name + " does not fill its row");
    S.n_listed_paths = n_listed;
    S.n_path_nodes = n_path_nodes;
    S.max_path_nodes = C[po::QK_MAXLEN];
    r->pp = po_paths_dims{n_b, n_inside, n_preds, n_listed, n_path_nodes};
    r->pp_n_total = R.n_total;
    (void)hipEventElapsedTime(&S.ms_chains, ev[0], ev[8]);
    (void)hipEventElapsedTime(&S.ms_count, ev[8], ev[9]);
    (void)hipEventElapsedTime(&S.ms_list, ev[9], ev[10]);
    (void)hipEventElapsedTime(&S.ms_total, ev[0], ev[10]);
    return PO_OK;
}

// ---- the contigs outside the bubble chains (po_layout_contigs, contigs.hip.h) ----------------------------------------------

// `cyclic`: po_layout_contigs_all -- without an exclude set the chains are those of po_layout_bubblechains_all.
po_status run_contigs(po_handle* h, po_result* graph, uint64_t min_len, uint32_t min_nodes, const uint8_t* exclude_in, uint32_t* contig_out,
                      uint32_t* pos_out, po_contig* table_out, uint64_t* n_contigs_out, bool cyclic = false) {
    const char* const name = cyclic ? "po_layout_contigs_all" : "po_layout_contigs";
    const int ev_first = cyclic ? EV_CONTIGS_ALL : EV_CONTIGS;
    hipStream_t st = h->stream;
    po_contig_stats& S = h->ctstats;
    S = po_contig_stats();
    DevBuf* B = h->d_ct;
    RankedGraph R;
    const size_t n_ids = h->len.size();
    uint32_t pad_e = 0;
    auto own = [&](size_t nn, size_t ne) -> po_status {
        pad_e = po::merge_sort_pad((uint32_t)ne);
        PO_TRY(ensure(h, B[CB_CNT], 128));
        PO_TRY(ensure(h, B[CB_EXCL], nn));
        PO_TRY(ensure(h, B[CB_LEN], (n_ids + 1) * 4));
        for (int k : {CB_INDEG, CB_OUTDEG, CB_INE}) PO_TRY(ensure(h, B[k], nn * 4));
        PO_TRY(ensure(h, B[CB_NLEN], nn * 8));
        for (int k : {CB_CLS, CB_OK0, CB_OK1, CB_KEPT}) PO_TRY(ensure(h, B[k], ne));
        for (int k : {CB_JB0, CB_JB1, CB_HOPS0, CB_HOPS1, CB_CJ0, CB_CJ1, CB_HEADOF, CB_PN, CB_PLAST, CB_CONTIGOUT, CB_POSOUT})
            PO_TRY(ensure(h, B[k], ne * 4));
        for (int k : {CB_WS0, CB_WS1, CB_PLEN}) PO_TRY(ensure(h, B[k], ne * 8));
        PO_TRY(ensure(h, B[CB_KEY], (size_t)pad_e * 8));
        PO_TRY(ensure(h, B[CB_VAL], (size_t)pad_e * 4));
        return ensure(h, B[CB_TABLE], (nn + ne) * sizeof(po::Contig));
    };
    // the ranks; without an exclude set the bubble chains too (their chain word per rank is the set)
    int e0 = 1;   // the event behind the stage run first
    if (exclude_in) {
        PO_TRY(ranked_open(h, graph, name, ev_first, po::KC_N, S, B[CB_INE], own, R));   // (the identity words: overwritten below)
    } else {
        BcWork W;
        po_superbubble_all_stats A = {};
        const po_status staged = cyclic ? bubblechain_stage(h, graph, name, ev_first, S, min_nodes, own, R, W, CyclicBubbles{A})
                                        : bubblechain_stage(h, graph, name, ev_first, S, min_nodes, own, R, W);
        S.n_chains = W.n_chains;
        S.n_batches = W.n_batches;
        PO_TRY(staged);
        e0 = W.ev_last + 2;
    }
    if (!R.ev) return PO_OK;
    const uint32_t n = R.n, n_order = R.n_order;
    if (!n_order) return PO_OK;
    hipEvent_t* ev = R.ev;
    unsigned long long *cnt = B[CB_CNT].as<unsigned long long>(), *ws[2] = {B[CB_WS0].as<unsigned long long>(), B[CB_WS1].as<unsigned long long>()},
                       *key = B[CB_KEY].as<unsigned long long>();
    uint8_t *excl = B[CB_EXCL].as<uint8_t>(), *cls = B[CB_CLS].as<uint8_t>(), *ok[2] = {B[CB_OK0].as<uint8_t>(), B[CB_OK1].as<uint8_t>()},
            *kept = B[CB_KEPT].as<uint8_t>();
    uint32_t *len = B[CB_LEN].as<uint32_t>(), *indeg = B[CB_INDEG].as<uint32_t>(), *outdeg = B[CB_OUTDEG].as<uint32_t>(),
             *ine = B[CB_INE].as<uint32_t>(), *jb[2] = {B[CB_JB0].as<uint32_t>(), B[CB_JB1].as<uint32_t>()},
             *hops[2] = {B[CB_HOPS0].as<uint32_t>(), B[CB_HOPS1].as<uint32_t>()}, *cj[2] = {B[CB_CJ0].as<uint32_t>(), B[CB_CJ1].as<uint32_t>()},
             *head_of = B[CB_HEADOF].as<uint32_t>(), *pn = B[CB_PN].as<uint32_t>(), *plast = B[CB_PLAST].as<uint32_t>(),
             *val = B[CB_VAL].as<uint32_t>(), *d_contig = B[CB_CONTIGOUT].as<uint32_t>(), *d_pos = B[CB_POSOUT].as<uint32_t>();
    long long *nlen = B[CB_NLEN].as<long long>(), *plen = B[CB_PLEN].as<long long>();
    po::Contig* table = B[CB_TABLE].as<po::Contig>();
    const po::Edge* edges = graph->d_rows.as<po::Edge>();
    volatile uint64_t* C = h->pinned + 48;   // this stage's counters on the host (words 16.. and 32.. are the scaffold's)
    auto counters_home = [&]() -> po_status {
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(h->pinned + 48, cnt, po::TK_N * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipStreamSynchronize(st));
        return PO_OK;
    };
    // degrees, the one in-edge, node lengths, the exclude bytes; class and link of every edge
    HIP_TRY(h, hipMemsetAsync(cnt, 0, 128, st));
    if (n_ids) HIP_TRY(h, hipMemcpyAsync(len, h->len.data(), n_ids * 4, hipMemcpyHostToDevice, st));
    if (exclude_in) HIP_TRY(h, hipMemcpyAsync(excl, exclude_in, n_order, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(po::k_ct_init, dim3(R.rank_grid), dim3(256), 0, st, n_order, R.val, (uint32_t)n_ids, R.n_total, len,
                       graph->merged ? graph->d_mlen.as<long long>() : (const long long*)nullptr,
                       exclude_in ? (const uint32_t*)nullptr : h->d_bc[HB_CHAINOUT].as<uint32_t>(), excl, indeg, outdeg, ine, nlen, cnt);
    if (n) {
        hipLaunchKernelGGL(po::k_ct_degrees, dim3(R.edge_grid), dim3(256), 0, st, R.ends, n, n_order, indeg, outdeg, ine);
        hipLaunchKernelGGL(po::k_ct_classes, dim3(R.edge_grid), dim3(256), 0, st, R.ends, n, n_order, indeg, outdeg, excl, cls, cnt);
        hipLaunchKernelGGL(po::k_ct_links, dim3(R.edge_grid), dim3(256), 0, st, R.ends, edges, n, n_order, ine, cls, jb[0], hops[0], ws[0]);
        HIP_TRY(h, hipMemsetAsync(pn, 0, (size_t)n * 4, st));
    }
    HIP_TRY(h, hipGetLastError());
    // (the caller's bytes were read by the copy above only once the stream got there)
    if (exclude_in) HIP_TRY(h, hipStreamSynchronize(st));
    RoundOps ops{h, st, R.rcnt};
    uint64_t ignored = 0;
    // list ranking of the extensions toward the head edge of their path: ping-pong, the last launch wrote buffer `fin`
    uint32_t launched = 0;
    if (n) {
        const int how = po::round_phase(ops, n, [&](uint32_t j) {
            const uint32_t a = launched & 1, b = a ^ 1;
            hipLaunchKernelGGL(po::k_ct_jump, dim3(R.edge_grid), dim3(256), 0, st, n, jb[a], hops[a], ws[a], jb[b], hops[b], ws[b], R.rcnt + j);
            ++launched;
        }, S.n_path_rounds, S.n_batches, ignored);
        if (how == po::ROUNDS_FAILED) HIP_TRY(h, ops.err != hipSuccess ? ops.err : hipErrorUnknown);
        if (how != po::ROUNDS_DONE) return fail(h, PO_ERR_HIP, std::string("internal: the ranking of ") + name + " reached its bound of edges + 2 rounds");
    }
    const uint32_t fin = launched & 1;
    HIP_TRY(h, hipEventRecord(ev[e0 + 1], st));
    // which late starts are covered: the same between two buffer pairs, over the heads
    launched = 0;
    if (n) {
        hipLaunchKernelGGL(po::k_ct_cover_init, dim3(R.edge_grid), dim3(256), 0, st, R.ends, n, n_order, ine, cls, jb[fin], cj[0], ok[0]);
        const int how = po::round_phase(ops, n, [&](uint32_t j) {
            const uint32_t a = launched & 1, b = a ^ 1;
            hipLaunchKernelGGL(po::k_ct_cover_jump, dim3(R.edge_grid), dim3(256), 0, st, n, cj[a], ok[a], cj[b], ok[b], R.rcnt + j);
            ++launched;
        }, S.n_cover_rounds, S.n_batches, ignored);
        if (how == po::ROUNDS_FAILED) HIP_TRY(h, ops.err != hipSuccess ? ops.err : hipErrorUnknown);
        if (how != po::ROUNDS_DONE) return fail(h, PO_ERR_HIP, std::string("internal: the coverage of ") + name + " reached its bound of edges + 2 rounds");
    }
    const uint32_t cfin = launched & 1;
    HIP_TRY(h, hipEventRecord(ev[e0 + 2], st));
    // the sums at the heads, the filter, the numbering: the free halves of the two ping-pongs take the two index arrays
    uint32_t *eidx = jb[fin ^ 1], *cidx = cj[cfin ^ 1];
    if (n) {
        hipLaunchKernelGGL(po::k_ct_paths, dim3(R.edge_grid), dim3(256), 0, st, R.ends, edges, n, n_order, indeg, outdeg, nlen, cls, jb[fin],
                           hops[fin], ws[fin], cj[cfin], ok[cfin], head_of, pn, plast, plen, cnt);
        hipLaunchKernelGGL(po::k_ct_filter, dim3(R.edge_grid), dim3(256), 0, st, n, (unsigned long long)min_len, head_of, pn, plen, kept, cnt);
    }
    hipLaunchKernelGGL(po::k_ct_isolated, dim3(R.rank_grid), dim3(256), 0, st, n_order, (unsigned long long)min_len, indeg, outdeg, nlen, R.root,
                       cnt);
    HIP_TRY(h, hipGetLastError());
    PO_TRY(prefix_sum<uint8_t>(h, kept, n, eidx, &h->pinned[2]));
    PO_TRY(prefix_sum<uint8_t>(h, R.root, n_order, R.index, &h->pinned[3]));
    PO_TRY(counters_home());
    S.n_excluded = C[po::TK_EXCLUDED];
    S.n_root_starts = C[po::TK_ROOT];
    S.n_late_starts = C[po::TK_LATE];
    S.n_blocked = C[po::TK_BLOCKED];
    S.n_covered_edges = C[po::TK_COVERED];
    S.n_uncovered_edges = C[po::TK_UNCOVERED];
    S.n_paths = C[po::TK_PATHS];
    S.n_short_paths = C[po::TK_SHORT];
    S.n_isolated = C[po::TK_ISO];
    S.n_short_isolated = C[po::TK_SHORTISO];
    S.max_path_nodes = C[po::TK_MAXN];
    const uint64_t n_kept64 = h->pinned[2], n_iso64 = h->pinned[3];
    if (C[po::TK_BAD]) return fail(h, PO_ERR_HIP, std::string("internal: a path of ") + name + " has no last edge");
    if (S.n_covered_edges + S.n_uncovered_edges != n || C[po::TK_PEDGES] != S.n_covered_edges || n_kept64 != C[po::TK_KEPT] ||
        n_kept64 + S.n_short_paths != S.n_paths || n_iso64 + S.n_short_isolated != S.n_isolated || S.n_paths > S.n_root_starts + S.n_late_starts ||
        S.n_root_starts + S.n_late_starts > n || S.n_isolated > n_order || S.max_path_nodes > (uint64_t)n + 1)
        return fail(h, PO_ERR_HIP, std::string("internal: the paths of ") + name + " do not add up");
    const uint32_t n_kept = (uint32_t)n_kept64, n_iso = (uint32_t)n_iso64;
    S.n_contigs = (uint64_t)n_kept + n_iso;
    if (n_kept) {
        const uint32_t pad = po::merge_sort_pad(n_kept);   // (<= pad_e: n_kept <= n)
        hipLaunchKernelGGL(po::k_ct_keys, dim3(stride_grid(h, std::max(n, pad))), dim3(256), 0, st, R.ends, n, n_kept, pad, kept, eidx, key, val);
        po::merge_sort_steps(n_kept, [&](uint32_t j, uint32_t k) {
            hipLaunchKernelGGL(po::k_merge_bitonic, dim3(cdiv(pad, 256)), dim3(256), 0, st, key, val, pad, j, k);
        });
        hipLaunchKernelGGL(po::k_ct_number, dim3(stride_grid(h, n_kept)), dim3(256), 0, st, R.ends, n, n_order, n_kept, val, R.val, pn, plast, plen,
                           cidx, table);
    }
    if (n_iso) hipLaunchKernelGGL(po::k_ct_iso_table, dim3(R.rank_grid), dim3(256), 0, st, n_order, n_kept, n_iso, R.root, R.index, R.val, nlen, table);
    if (n) hipLaunchKernelGGL(po::k_ct_edge_out, dim3(R.edge_grid), dim3(256), 0, st, n, head_of, kept, cidx, hops[fin], d_contig, d_pos);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(ev[e0 + 3], st));
    static_assert(sizeof(po_contig) == sizeof(po::Contig) && sizeof(po_contig) == 24, "po_contig is the device's table entry");
    PO_TRY(land_outputs(h, {{table, (size_t)S.n_contigs * sizeof(po_contig), table_out}, {d_contig, (size_t)n * 4, contig_out},
                            {d_pos, (size_t)n * 4, pos_out}}, cnt, po::TK_N));
    *n_contigs_out = S.n_contigs;
    if (!exclude_in) (void)hipEventElapsedTime(&S.ms_bubblechains, ev[0], ev[e0]);
    (void)hipEventElapsedTime(&S.ms_ranks, ev[0], ev[1]);
    (void)hipEventElapsedTime(&S.ms_paths, ev[e0], ev[e0 + 1]);
    (void)hipEventElapsedTime(&S.ms_cover, ev[e0 + 1], ev[e0 + 2]);
    (void)hipEventElapsedTime(&S.ms_label, ev[e0 + 2], ev[e0 + 3]);
    (void)hipEventElapsedTime(&S.ms_total, ev[0], ev[e0 + 3]);
    return PO_OK;
}

// ---- scoring and pruning of the haplotype extensions at one bubble (po_phase_branch, phase.hip.h) ----------------------------

// offsets of a CSR: they start at 0 and never decrease
bool phase_offsets_ok(const uint32_t* off, uint64_t n_lists) {
    if (off[0] != 0) return false;
    for (uint64_t i = 0; i < n_lists; ++i)
        if (off[i + 1] < off[i]) return false;
    return true;
}

// The checks of po_phase_branch in front of the device, in the order the header lists them: the sentence of the first one
// that fails, empty when the call may go on (Pk = P^k then).
std::string phase_check(const po_phase_params& p, const po_phase_input& in, uint64_t& Pk, const char* who = "po_phase_branch") {
    const std::string name = std::string(who) + ": ";
    if (p.reserved || p.reserved2 || !(p.threshold >= 0.0) || p.n_levels > po::PH_MAX_LEVELS) return name + "bad parameters";
    if (p.ploidy < 1 || p.ploidy > po::PH_MAX_K) return name + "the ploidy must be 1 to 8";
    if (p.n_paths < 1 || p.n_paths > po::PH_MAX_P) return name + "the number of paths must be 1 to 64";
    if (!p.n_cands) return name + "there must be at least one candidate set";
    Pk = 1;
    for (uint32_t i = 0; i < p.ploidy; ++i) Pk *= p.n_paths;   // (at most 2^48)
    if (Pk >= (1ull << 31) || Pk * p.n_cands >= (1ull << 31)) return name + "too many extensions for one call";
    const uint64_t n_slots = (uint64_t)p.n_cands * p.ploidy;
    if ((p.n_reads && (!in.overlap_max || !in.aln_off)) || !in.path_off || !in.set_off || (p.prune && p.n_levels && !in.levels))
        return name + "an input array is missing";
    if (p.n_reads && !phase_offsets_ok(in.aln_off, p.n_reads)) return name + "the offsets of the alignments do not start at 0 or decrease";
    if (!phase_offsets_ok(in.path_off, p.n_paths)) return name + "the offsets of the paths do not start at 0 or decrease";
    if (!phase_offsets_ok(in.set_off, n_slots)) return name + "the offsets of the read sets do not start at 0 or decrease";
    const uint32_t n_aln = p.n_reads ? in.aln_off[p.n_reads] : 0, n_pids = in.path_off[p.n_paths], n_sids = in.set_off[n_slots];
    if ((n_aln && (!in.aln_b || !in.aln_a0 || !in.aln_a1)) || (n_pids && !in.path_ids) || (n_sids && !in.set_ids))
        return name + "an input array is missing";
    for (uint32_t j = 0; j < n_aln; ++j)
        if (in.aln_b[j] >= p.n_b) return name + "a local read id is not below n_b";
    for (uint32_t j = 0; j < n_pids; ++j)
        if (in.path_ids[j] >= p.n_b) return name + "a local read id is not below n_b";
    for (uint32_t j = 0; j < n_sids; ++j)
        if (in.set_ids[j] >= p.n_b) return name + "a local read id is not below n_b";
    return std::string();
}

// the read sets of a walk (po_walk_step) in place of set_off / set_ids: bit rows of W words over ids below nb
struct WalkRows {
    const uint32_t* rows;
    uint32_t W, nb;
};

// the inputs of a step that are on the device already (po_walk_step_resident): used where they lie, nothing of them goes up
struct PhaseDev {
    const int32_t* om;
    const uint32_t *aln_off, *aln_b;
    const int32_t *a0, *a1;
    const uint32_t* pids;
    uint32_t n_aln, n_pids;
};

po_status run_phase(po_handle* h, const po_phase_params& p, const po_phase_input& in, uint32_t Pk, uint32_t* cand_out, uint32_t* ext_out,
                    double* rl_out, uint64_t cap, double* table_out, uint64_t* n_out, const WalkRows* walk = nullptr,
                    const PhaseDev* dev = nullptr) {
    const char* const name = dev ? "po_walk_step_resident" : walk ? "po_walk_step" : "po_phase_branch";
    h->ph_fcand = h->ph_fext = h->ph_pbits = nullptr;
    h->ph_frl = nullptr;
    hipStream_t st = h->stream;
    po_phase_stats& S = h->phstats;
    S = po_phase_stats();
    S.level_used = -1;
    S.max_rl = std::nan("");
    S.n_levels = p.prune ? p.n_levels : 0;
    DevBuf* B = h->d_ph;
    const uint32_t k = p.ploidy, P = p.n_paths, C = p.n_cands, R = p.n_reads, nb = p.n_b, W = std::max(1u, cdiv(nb, 32));
    const uint32_t N = C * Pk, n_slots = C * k;   // (both below 2^31: phase_check)
    const uint32_t n_aln = dev ? dev->n_aln : (R ? in.aln_off[R] : 0), n_pids = dev ? dev->n_pids : in.path_off[P], n_sids = in.set_off[n_slots];
    const size_t Rr = std::max<size_t>(R, 1);
    PO_TRY(lay_events(h));
    hipEvent_t* ev = h->ev_lay + EV_PHASE;
    // everything whose size the inputs give, before the first launch (the two lists follow once their lengths are known)
    PO_TRY(ensure(h, h->d_scalars, 128));
    PO_TRY(ensure(h, B[FB_CNT], 128));
    PO_TRY(ensure(h, B[FB_HIST], (po::PH_MAX_LEVELS + 1) * 8));
    PO_TRY(ensure(h, B[FB_LEVELS], po::PH_MAX_LEVELS * 8));
    if (!dev) {
        for (int b : {FB_OM, FB_ALNOFF}) PO_TRY(ensure(h, B[b], ((size_t)R + 1) * 4));
        for (int b : {FB_ALNB, FB_A0, FB_A1}) PO_TRY(ensure(h, B[b], ((size_t)n_aln + 1) * 4));
        PO_TRY(ensure(h, B[FB_PIDS], ((size_t)n_pids + 1) * 4));
    }
    PO_TRY(ensure(h, B[FB_POFF], ((size_t)P + 1) * 4));
    PO_TRY(ensure(h, B[FB_SOFF], ((size_t)n_slots + 1) * 4));
    PO_TRY(ensure(h, B[FB_SIDS], ((size_t)n_sids + 1) * 4));
    if (!walk) PO_TRY(ensure(h, B[FB_SBITS], (size_t)n_slots * W * 4));
    PO_TRY(ensure(h, B[FB_PBITS], (size_t)P * W * 4));
    PO_TRY(ensure(h, B[FB_SIV], (size_t)n_slots * Rr * sizeof(po::PhInterval)));
    PO_TRY(ensure(h, B[FB_PIV], (size_t)P * Rr * sizeof(po::PhInterval)));
    PO_TRY(ensure(h, B[FB_TABLE], (size_t)n_slots * P * 8));
    PO_TRY(ensure(h, B[FB_RL], (size_t)N * 8));
    PO_TRY(ensure(h, B[FB_KEEP], N));
    PO_TRY(ensure(h, B[FB_PLACE], (size_t)N * 4));
    unsigned long long *cnt = B[FB_CNT].as<unsigned long long>(), *hist = B[FB_HIST].as<unsigned long long>();
    // (with `dev` the five arrays of the alignments and the path ids are read where the gather and the k_rs_ kernels left them)
    int32_t *om = dev ? const_cast<int32_t*>(dev->om) : B[FB_OM].as<int32_t>(), *a0 = dev ? const_cast<int32_t*>(dev->a0) : B[FB_A0].as<int32_t>(),
            *a1 = dev ? const_cast<int32_t*>(dev->a1) : B[FB_A1].as<int32_t>();
    uint32_t *aln_off = dev ? const_cast<uint32_t*>(dev->aln_off) : B[FB_ALNOFF].as<uint32_t>(),
             *aln_b = dev ? const_cast<uint32_t*>(dev->aln_b) : B[FB_ALNB].as<uint32_t>(), *poff = B[FB_POFF].as<uint32_t>(),
             *pids = dev ? const_cast<uint32_t*>(dev->pids) : B[FB_PIDS].as<uint32_t>(), *soff = B[FB_SOFF].as<uint32_t>(), *sids = B[FB_SIDS].as<uint32_t>(),
             *sbits = B[FB_SBITS].as<uint32_t>(), *pbits = B[FB_PBITS].as<uint32_t>(), *place = B[FB_PLACE].as<uint32_t>();
    po::PhInterval *siv = B[FB_SIV].as<po::PhInterval>(), *piv = B[FB_PIV].as<po::PhInterval>();
    double *table = B[FB_TABLE].as<double>(), *rl = B[FB_RL].as<double>(), *levels = B[FB_LEVELS].as<double>();
    uint8_t* keep = B[FB_KEEP].as<uint8_t>();
    HIP_TRY(h, hipEventRecord(ev[0], st));
    HIP_TRY(h, hipMemsetAsync(cnt, 0, 128, st));
    if (!walk) HIP_TRY(h, hipMemsetAsync(sbits, 0, (size_t)n_slots * W * 4, st));
    HIP_TRY(h, hipMemsetAsync(pbits, 0, (size_t)P * W * 4, st));
    auto up = [&](void* dst, const void* src, size_t bytes) -> po_status {
        if (bytes) HIP_TRY(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st));
        return PO_OK;
    };
    if (!dev) {
        PO_TRY(up(om, in.overlap_max, (size_t)R * 4));
        PO_TRY(up(aln_off, in.aln_off, R ? ((size_t)R + 1) * 4 : 0));
        PO_TRY(up(aln_b, in.aln_b, (size_t)n_aln * 4));
        PO_TRY(up(a0, in.aln_a0, (size_t)n_aln * 4));
        PO_TRY(up(a1, in.aln_a1, (size_t)n_aln * 4));
        PO_TRY(up(pids, in.path_ids, (size_t)n_pids * 4));
    }
    PO_TRY(up(poff, in.path_off, ((size_t)P + 1) * 4));
    if (!walk) {
        PO_TRY(up(soff, in.set_off, ((size_t)n_slots + 1) * 4));
        PO_TRY(up(sids, in.set_ids, (size_t)n_sids * 4));
    }
    // the bitsets, the interval of every (read set, read) and (path, read)
    if (!walk) hipLaunchKernelGGL(po::k_ph_bits, dim3(stride_grid(h, n_slots)), dim3(256), 0, st, n_slots, soff, sids, nb, W, sbits);
    hipLaunchKernelGGL(po::k_ph_bits, dim3(stride_grid(h, P)), dim3(256), 0, st, P, poff, pids, nb, W, pbits);
    if (R) {
        // (a walk's rows are shorter than this call's: ids at or past their length read as 0)
        hipLaunchKernelGGL(po::k_ph_intervals, dim3(stride_grid(h, (uint64_t)n_slots * R)), dim3(256), 0, st, n_slots, R, walk ? walk->nb : nb,
                           walk ? walk->W : W, walk ? walk->rows : sbits, aln_off, aln_b, a0, a1, om, siv);
        hipLaunchKernelGGL(po::k_ph_intervals, dim3(stride_grid(h, (uint64_t)P * R)), dim3(256), 0, st, P, R, nb, W, pbits, aln_off, aln_b, a0, a1,
                           om, piv);
    }
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(ev[1], st));
    const uint32_t wg_cap = (uint32_t)h->n_cu * 8;
    hipLaunchKernelGGL(po::k_ph_table, dim3(std::min(n_slots, wg_cap)), dim3(256), 0, st, n_slots, P, R, siv, piv, om, table);
    HIP_TRY(h, hipEventRecord(ev[2], st));
    // rl and keep byte of every extension id
    po::PhExtend X;
    X.C = C;
    X.P = P;
    X.k = k;
    X.Pk = Pk;
    X.chunks = cdiv(Pk, 256);
    X.start_mode = p.start_of_block != 0;
    X.dead = R < p.min_spanning_reads;
    X.kfact = 1;
    for (uint32_t i = 2; i <= k; ++i) X.kfact *= i;
    X.denom = (double)k * (double)R;
    X.log_thr = p.threshold == 0.0 ? -(double)INFINITY : std::log10(p.threshold);
    hipLaunchKernelGGL(po::k_ph_extend, dim3(std::min(C * X.chunks, wg_cap)), dim3(256), 0, st, X, table, rl, keep, cnt);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(ev[3], st));
    // the kept list: places by prefix sum, the entries to their places, the greatest rl on the way
    PO_TRY(prefix_sum<uint8_t>(h, keep, N, place, &h->pinned[2]));
    HIP_TRY(h, hipMemcpyAsync(h->pinned + 16, cnt, po::PK_N * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    const uint64_t n_kept64 = h->pinned[2];
    S.n_extensions = h->pinned[16 + po::PK_ENUM];
    S.n_kept = S.n_survivors = n_kept64;
    if (n_kept64 != h->pinned[16 + po::PK_KEPT] || n_kept64 > S.n_extensions || S.n_extensions > N)
        return fail(h, PO_ERR_HIP, std::string("internal: the extensions of ") + name + " do not add up");
    const uint32_t n_kept = (uint32_t)n_kept64;
    for (int b : {FB_KCAND, FB_KEXT, FB_PLACE2}) PO_TRY(ensure(h, B[b], ((size_t)n_kept + 1) * 4));
    PO_TRY(ensure(h, B[FB_KRL], ((size_t)n_kept + 1) * 8));
    PO_TRY(ensure(h, B[FB_KEEP2], (size_t)n_kept + 1));
    uint32_t *kcand = B[FB_KCAND].as<uint32_t>(), *kext = B[FB_KEXT].as<uint32_t>(), *place2 = B[FB_PLACE2].as<uint32_t>();
    double* krl = B[FB_KRL].as<double>();
    uint8_t* keep2 = B[FB_KEEP2].as<uint8_t>();
    double max_rl = std::nan("");
    if (n_kept) {
        hipLaunchKernelGGL(po::k_ph_gather, dim3(stride_grid(h, N)), dim3(256), 0, st, N, n_kept, Pk, keep, place, (const uint32_t*)nullptr,
                           (const uint32_t*)nullptr, rl, kcand, kext, krl, cnt + po::PK_N);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(h->pinned + 18, cnt + po::PK_N, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipEventRecord(ev[4], st));
        HIP_TRY(h, hipStreamSynchronize(st));
        const uint64_t key = h->pinned[18];
        if (!key) return fail(h, PO_ERR_HIP, std::string("internal: the kept list of ") + name + " has no greatest entry");
        const uint64_t bits = (key >> 63) ? (key & 0x7FFFFFFFFFFFFFFFull) : ~key;
        std::memcpy(&max_rl, &bits, 8);
    } else {
        HIP_TRY(h, hipEventRecord(ev[4], st));
    }
    S.max_rl = max_rl;
    // prune: the survivors of every level in one pass, the level the reference's loop stops at, its survivors in order
    const uint32_t *fcand = kcand, *fext = kext;
    const double* frl = krl;
    uint32_t n_final = n_kept;
    if (p.prune && n_kept >= 2 && p.n_levels && max_rl != -(double)INFINITY) {
        const uint32_t L = p.n_levels;
        std::vector<double> lv(in.levels, in.levels + L);
        for (uint32_t j = 1; j < L; ++j) lv[j] = lv[j] >= lv[j - 1] ? lv[j] : lv[j - 1];   // surviving levels 0..j = surviving their greatest
        HIP_TRY(h, hipMemcpyAsync(levels, lv.data(), (size_t)L * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(h, hipMemsetAsync(hist, 0, ((size_t)L + 1) * 8, st));
        PO_TRY(ensure_host(h, h->scratch_host, ((size_t)L + 1) * 8));
        hipLaunchKernelGGL(po::k_ph_levels, dim3(stride_grid(h, n_kept)), dim3(256), 0, st, n_kept, krl, max_rl, levels, L, hist);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(h->scratch_host.p, hist, ((size_t)L + 1) * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipStreamSynchronize(st));
        const uint64_t* hh = static_cast<const uint64_t*>(h->scratch_host.p);   // hh[t]: the entries that survive exactly t levels
        std::vector<uint64_t> left(L);
        uint64_t behind = 0, all = hh[0];
        for (uint32_t j = L; j-- > 0;) {
            behind += hh[j + 1];
            left[j] = behind;
            all += hh[j + 1];
        }
        if (all != n_kept) return fail(h, PO_ERR_HIP, std::string("internal: the prune levels of ") + name + " do not add up");
        uint32_t used = L - 1;
        for (uint32_t j = 0; j < L; ++j)
            if (left[j] <= p.max_candidates) {
                used = j;
                break;
            }
        for (uint32_t j = 0; j < L && j < 16; ++j) S.level_counts[j] = left[j];
        S.level_used = (int32_t)used;
        hipLaunchKernelGGL(po::k_ph_survive, dim3(stride_grid(h, n_kept)), dim3(256), 0, st, n_kept, krl, max_rl, lv[used], keep2);
        HIP_TRY(h, hipGetLastError());
        PO_TRY(prefix_sum<uint8_t>(h, keep2, n_kept, place2, &h->pinned[3]));
        HIP_TRY(h, hipStreamSynchronize(st));
        const uint64_t n_left = h->pinned[3];
        if (n_left != left[used]) return fail(h, PO_ERR_HIP, std::string("internal: the survivors of ") + name + " do not add up");
        for (int b : {FB_SCAND, FB_SEXT}) PO_TRY(ensure(h, B[b], ((size_t)n_left + 1) * 4));
        PO_TRY(ensure(h, B[FB_SRL], ((size_t)n_left + 1) * 8));
        if (n_left)
            hipLaunchKernelGGL(po::k_ph_gather, dim3(stride_grid(h, n_kept)), dim3(256), 0, st, n_kept, (uint32_t)n_left, Pk, keep2, place2, kcand,
                               kext, krl, B[FB_SCAND].as<uint32_t>(), B[FB_SEXT].as<uint32_t>(), B[FB_SRL].as<double>(),
                               (unsigned long long*)nullptr);
        HIP_TRY(h, hipGetLastError());
        fcand = B[FB_SCAND].as<uint32_t>();
        fext = B[FB_SEXT].as<uint32_t>();
        frl = B[FB_SRL].as<double>();
        n_final = (uint32_t)n_left;
        S.n_survivors = n_left;
    }
    HIP_TRY(h, hipEventRecord(ev[5], st));
    const size_t n_give = (size_t)std::min<uint64_t>(cap, n_final);
    PO_TRY(land_outputs(h, {{fcand, n_give * 4, cand_out}, {fext, n_give * 4, ext_out}, {frl, n_give * 8, rl_out},
                            {table, (size_t)n_slots * P * 8, table_out}}, cnt, po::PK_N));
    *n_out = n_final;
    h->ph_fcand = fcand;
    h->ph_fext = fext;
    h->ph_frl = frl;
    h->ph_pbits = pbits;
    (void)hipEventElapsedTime(&S.ms_intervals, ev[0], ev[1]);
    (void)hipEventElapsedTime(&S.ms_table, ev[1], ev[2]);
    (void)hipEventElapsedTime(&S.ms_extend, ev[2], ev[3]);
    (void)hipEventElapsedTime(&S.ms_filter, ev[3], ev[4]);
    (void)hipEventElapsedTime(&S.ms_prune, ev[4], ev[5]);
    (void)hipEventElapsedTime(&S.ms_total, ev[0], ev[5]);
    return PO_OK;
}

// ---- every listed path of a large bubble scored, the best of them named (po_phase_large, large.hip.h) ------------------------

// The checks of po_phase_large that need neither the result nor the device, in the order the header lists them: the sentence
// of the first one that fails, empty when the call may go on.
std::string large_check(const po_large_params& p, const po_large_input& in) {
    const std::string name = "po_phase_large: ";
    if (p.reserved) return name + "bad parameters";
    if (p.n_best < 1 || p.n_best > po::LG_MAX_BEST) return name + "n_best must be 1 to 8";
    if (!p.n_reads) return name + "there must be at least one relevant read";
    if (!in.overlap_max || !in.aln_off || !in.node_off) return name + "an input array is missing";
    if (!phase_offsets_ok(in.aln_off, p.n_reads)) return name + "the offsets of the alignments do not start at 0 or decrease";
    if (!phase_offsets_ok(in.node_off, in.n_nodes)) return name + "the offsets of the interior nodes do not start at 0 or decrease";
    const uint32_t n_aln = in.aln_off[p.n_reads], n_ids = in.node_off[in.n_nodes];
    if ((n_aln && (!in.aln_b || !in.aln_a0 || !in.aln_a1)) || (n_ids && !in.node_ids)) return name + "an input array is missing";
    for (uint32_t j = 0; j < n_aln; ++j)
        if (in.aln_b[j] >= p.n_b) return name + "a local read id is not below n_b";
    for (uint32_t j = 0; j < n_ids; ++j)
        if (in.node_ids[j] >= p.n_b) return name + "a local read id is not below n_b";
    return std::string();
}

// the table, inside_off and bubble_path_off of a paths result on the host (they are bubble-sized), fetched once
po_status paths_home(po_handle* h, po_result* r) {
    const size_t nb = (size_t)r->pp.n_bubbles;
    if (r->pp_table.size() == nb && r->pp_bpo.size() == nb + 1) return PO_OK;
    std::vector<po_bubble_paths> table(nb);
    std::vector<uint32_t> inoff(nb + 1, 0u), bpo(nb + 1, 0u);
    if (nb) {
        hipStream_t st = h->stream;
        HIP_TRY(h, hipMemcpyAsync(table.data(), r->d_pp[PR_TABLE].p, nb * sizeof(po_bubble_paths), hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipMemcpyAsync(inoff.data(), r->d_pp[PR_INOFF].p, (nb + 1) * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipMemcpyAsync(bpo.data(), r->d_pp[PR_BPO].p, (nb + 1) * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipStreamSynchronize(st));
    }
    r->pp_table.swap(table);
    r->pp_inoff.swap(inoff);
    r->pp_bpo.swap(bpo);
    return PO_OK;
}

po_status run_large(po_handle* h, po_result* r, const po_large_params& p, const po_large_input& in, uint64_t* best_out, double* best_score_out,
                    double* scores_out, uint32_t* n_best_out) {
    const std::string name = "po_phase_large: ";
    hipStream_t st = h->stream;
    po_large_stats& S = h->lgstats;
    S = po_large_stats();
    PO_TRY(paths_home(h, r));
    const po_bubble_paths& T = r->pp_table[p.bubble];
    if (T.flags & PO_PATHS_UNLISTED)
        return fail(h, PO_ERR_INVALID, name + "the paths of bubble " + std::to_string(p.bubble) + " were not listed (more than max_paths)");
    if (in.n_nodes != T.n_inside)
        return fail(h, PO_ERR_INVALID, name + "n_nodes is " + std::to_string(in.n_nodes) + ", bubble " + std::to_string(p.bubble) + " has " +
                                           std::to_string(T.n_inside) + " interior nodes");
    const uint32_t first = r->pp_bpo[p.bubble], P = r->pp_bpo[p.bubble + 1] - first, in_first = r->pp_inoff[p.bubble];
    const uint32_t n_inside = T.n_inside, R = p.n_reads, nb = p.n_b, W = std::max(1u, cdiv(nb, 32)), n_total = r->pp_n_total;
    if (P != T.n_paths || r->pp_inoff[p.bubble + 1] - in_first != n_inside || (uint64_t)first + P > r->pp.n_listed_paths)
        return fail(h, PO_ERR_HIP, "internal: the table of the paths result of po_phase_large does not add up");
    const uint32_t n_aln = in.aln_off[R], n_ids = in.node_off[n_inside];
    DevBuf* B = h->d_lg;
    PO_TRY(lay_events(h));
    hipEvent_t* ev = h->ev_lay + EV_LARGE;
    // everything is sized by the inputs and allocated before the first launch
    PO_TRY(ensure(h, B[LB_CNT], 256));
    for (int b : {LB_OM, LB_ALNOFF}) PO_TRY(ensure(h, B[b], ((size_t)R + 1) * 4));
    for (int b : {LB_ALNB, LB_A0, LB_A1}) PO_TRY(ensure(h, B[b], ((size_t)n_aln + 1) * 4));
    PO_TRY(ensure(h, B[LB_NOFF], ((size_t)n_inside + 1) * 4));
    PO_TRY(ensure(h, B[LB_NIDS], ((size_t)n_ids + 1) * 4));
    PO_TRY(ensure(h, B[LB_NBITS], std::max<size_t>((size_t)n_inside * W * 4, 256)));
    PO_TRY(ensure(h, B[LB_NIV], std::max<size_t>((size_t)n_inside * R * sizeof(po::PhInterval), 256)));
    PO_TRY(ensure(h, B[LB_SLOT], ((size_t)n_total + 1) * 4));
    PO_TRY(ensure(h, B[LB_SCORE], ((size_t)P + 1) * 8));
    unsigned long long* cnt = B[LB_CNT].as<unsigned long long>();
    int32_t *om = B[LB_OM].as<int32_t>(), *a0 = B[LB_A0].as<int32_t>(), *a1 = B[LB_A1].as<int32_t>();
    uint32_t *aln_off = B[LB_ALNOFF].as<uint32_t>(), *aln_b = B[LB_ALNB].as<uint32_t>(), *noff = B[LB_NOFF].as<uint32_t>(),
             *nids = B[LB_NIDS].as<uint32_t>(), *nbits = B[LB_NBITS].as<uint32_t>(), *slot_of = B[LB_SLOT].as<uint32_t>();
    po::PhInterval* niv = B[LB_NIV].as<po::PhInterval>();
    double* score = B[LB_SCORE].as<double>();
    const uint32_t *poff = r->d_pp[PR_POFF].as<uint32_t>() + first, *path_nodes = r->d_pp[PR_PATHS].as<uint32_t>(),
                   *inside_nodes = r->d_pp[PR_INNODES].as<uint32_t>() + in_first;
    HIP_TRY(h, hipEventRecord(ev[0], st));
    static_assert(po::LK_N * 8 <= 256, "the counters of po_phase_large fit their buffer");
    HIP_TRY(h, hipMemsetAsync(cnt, 0, (size_t)po::LK_BEST * 8, st));
    HIP_TRY(h, hipMemsetAsync(cnt + po::LK_BEST, 0xFF, (size_t)po::LG_MAX_BEST * 8, st));   // (LG_NO_INDEX)
    HIP_TRY(h, hipMemsetAsync(slot_of, 0xFF, ((size_t)n_total + 1) * 4, st));               // (LG_NO_SLOT)
    HIP_TRY(h, hipMemsetAsync(nbits, 0, std::max<size_t>((size_t)n_inside * W * 4, 4), st));
    auto up = [&](void* dst, const void* src, size_t bytes) -> po_status {
        if (bytes) HIP_TRY(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st));
        return PO_OK;
    };
    PO_TRY(up(om, in.overlap_max, (size_t)R * 4));
    PO_TRY(up(aln_off, in.aln_off, ((size_t)R + 1) * 4));
    PO_TRY(up(aln_b, in.aln_b, (size_t)n_aln * 4));
    PO_TRY(up(a0, in.aln_a0, (size_t)n_aln * 4));
    PO_TRY(up(a1, in.aln_a1, (size_t)n_aln * 4));
    PO_TRY(up(noff, in.node_off, ((size_t)n_inside + 1) * 4));
    PO_TRY(up(nids, in.node_ids, (size_t)n_ids * 4));
    if (n_inside) {
        hipLaunchKernelGGL(po::k_lg_slots, dim3(stride_grid(h, n_inside)), dim3(256), 0, st, n_inside, inside_nodes, n_total, slot_of);
        hipLaunchKernelGGL(po::k_ph_bits, dim3(stride_grid(h, n_inside)), dim3(256), 0, st, n_inside, noff, nids, nb, W, nbits);
        hipLaunchKernelGGL(po::k_ph_intervals, dim3(stride_grid(h, (uint64_t)n_inside * R)), dim3(256), 0, st, n_inside, R, nb, W, nbits, aln_off,
                           aln_b, a0, a1, om, niv);
    }
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(ev[1], st));
    const uint32_t wg_cap = large_grid_cap(h);
    hipLaunchKernelGGL(po::k_lg_score, dim3(std::max(1u, std::min(P, wg_cap))), dim3(256), 0, st, P, R, n_inside, n_total, poff, path_nodes, slot_of,
                       niv, om, score, cnt);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(ev[2], st));
    const uint32_t n_best = (uint32_t)std::min<uint64_t>(p.n_best, P);
    for (uint32_t j = 0; j < n_best; ++j) {
        hipLaunchKernelGGL(po::k_lg_best_key, dim3(stride_grid(h, P)), dim3(256), 0, st, P, j, score, cnt);
        hipLaunchKernelGGL(po::k_lg_best_idx, dim3(stride_grid(h, P)), dim3(256), 0, st, P, j, score, cnt);
    }
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(ev[3], st));
    PO_TRY(land_outputs(h, {{score, (size_t)P * 8, scores_out}}, cnt, po::LK_N));
    const volatile uint64_t* C = h->pinned + 16;
    for (uint32_t j = 0; j < n_best; ++j) {
        const uint64_t key = C[po::LK_KEY + j], at = C[po::LK_BEST + j];
        if (!key || at >= P) return fail(h, PO_ERR_HIP, "internal: the selection of po_phase_large found no path");
        for (uint32_t i = 0; i < j; ++i)
            if (C[po::LK_BEST + i] == at) return fail(h, PO_ERR_HIP, "internal: the selection of po_phase_large named a path twice");
        const uint64_t bits = (key >> 63) ? (key & 0x7FFFFFFFFFFFFFFFull) : ~key;
        if (best_out) best_out[j] = at;
        if (best_score_out) std::memcpy(best_score_out + j, &bits, 8);
    }
    *n_best_out = n_best;
    S.n_paths = P;
    S.n_inside = n_inside;
    S.n_reads = R;
    S.max_path_nodes = C[po::LK_MAXLEN];
    (void)hipEventElapsedTime(&S.ms_intervals, ev[0], ev[1]);
    (void)hipEventElapsedTime(&S.ms_score, ev[1], ev[2]);
    (void)hipEventElapsedTime(&S.ms_best, ev[2], ev[3]);
    (void)hipEventElapsedTime(&S.ms_total, ev[0], ev[3]);
    return PO_OK;
}

// ---- the candidate sets of a walk along a bubble chain, resident on the device (po_walk_*, walk.hip.h) -----------------------

constexpr uint8_t WALK_KIND = 5;   // po_result::special of a walk

// A buffer of a walk that must hold at least `need` bytes and KEEP its first `used` bytes (ensure() grows without them).
// It belongs to a result, so it never comes out of the handle's arena.
po_status walk_grow(po_handle* h, DevBuf& b, size_t used, size_t need) {
    if (need <= b.cap) return PO_OK;
    DevBuf bigger;
    PO_TRY(ensure(h, bigger, need + need / 2, 1.0, false));
    if (used) {
        hipError_t e = hipMemcpyAsync(bigger.p, b.p, used, hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) {
            bigger.release();
            return fail(h, PO_ERR_HIP, std::string("po_walk_step: keeping the links of the walk: ") + hipGetErrorString(e));
        }
    }
    b.release();
    b = bigger;
    return PO_OK;
}

void walk_clear(po_result* w) {
    w->wk_n_cands = 1;
    w->wk_W = 0;
    w->wk_level_off.clear();
    w->wk_reads.clear();
    w->wk_sorted.clear();
    // the resident route: nothing on the device is touched here -- the next device call un-maps the old block and clears the sets
    w->wk_route = 0;
    if (w->rs_n_block) {
        w->rs_unmap_n = w->rs_n_block;
        w->rs_n_block = 0;
    }
    w->rs_clear_prev = w->d_rs_prev.p != nullptr;
    w->rs_prevg_bound = 0;
    if (po_result* g = w->rs_live) {
        // new_block() and the step on the same relevant reads: a gather that fell back (or took every aligning read) lives on, once
        if ((g->rv.fell_back || g->rv_mode == 1) && g->rv_resets == 0) {
            g->rv_resets = 1;
            g->rv_depth = 0;
        } else {
            g->rv_stale = true;
            g->rv_walk = nullptr;   // (neither knows of the other any more: either may be freed first)
            w->rs_live = nullptr;
        }
    }
}

inline uint32_t walk_depth(const po_result* w) { return w->wk_level_off.empty() ? 0u : (uint32_t)(w->wk_level_off.size() - 1); }

// The checks of po_walk_step that po_phase_branch does not have, in the order the header lists them.
std::string walk_check(const po_handle* h, const po_result* w, const po_phase_params& p, const po_phase_input& in, const uint32_t* b_reads) {
    const std::string name = "po_walk_step: ";
    if (w->special != WALK_KIND) return name + "needs the result of po_walk_create";
    if (w->h != h) return name + "the walk belongs to another handle";
    if (in.set_off || in.set_ids) return name + "set_off and set_ids must be NULL: the read sets are the walk's";
    if (p.ploidy != w->wk_k) return name + "the ploidy is not the walk's";
    if (p.n_cands != w->wk_n_cands) return name + "n_cands is not the number of candidates the walk holds";
    if ((p.start_of_block != 0) != (walk_depth(w) == 0)) return name + "start_of_block is not the walk's";
    if (w->wk_route == 2) return name + "the block advanced by po_walk_step_resident: the two routes do not mix before po_walk_reset";
    if (p.n_b && !b_reads) return name + "b_reads is missing";
    for (uint32_t j = 1; j < p.n_b; ++j)
        if (b_reads[j] <= b_reads[j - 1]) return name + "b_reads is not strictly ascending";
    return std::string();
}

// what the three calls that ask a walk check first: the sentence, empty when the call may go on
std::string walk_asked(const po_result* walk, const char* who, const uint32_t* cands, uint64_t n) {
    const std::string name = std::string(who) + ": ";
    if (walk->special != WALK_KIND) return std::string(who) + " needs the result of po_walk_create";
    if (n >= (1ull << 31)) return name + "too many candidates named in one call";
    if (n && !cands) return name + "the candidates are missing";
    for (uint64_t q = 0; q < n; ++q)
        if (cands[q] >= walk->wk_n_cands) return name + "a candidate is not below the number the walk holds";
    return std::string();
}

// The final list of the step that has just run becomes the walk's candidates: the other half of each ping-pong pair takes the
// new state (k_wk_advance); nothing of the live half changes before the launch has succeeded.  `also` launches what a route
// commits beside it, in front of the one synchronise.  What maps the block's reads is the caller's.
template <class Also>
po_status walk_take_over(po_handle* h, po_result* w, const WalkRows& rows, uint32_t C, uint32_t P, uint32_t nb, uint32_t n_new, Also&& also) {
    hipStream_t st = h->stream;
    po_walk_stats& S = h->wkstats;
    const uint32_t k = w->wk_k, W_new = std::max(1u, cdiv(nb, 32)), depth = walk_depth(w);
    const int nxt = w->wk_cur ^ 1;
    const uint64_t links_used = depth ? w->wk_level_off[depth] : 0;
    PO_TRY(ensure(h, w->d_wk_rows[nxt], (size_t)n_new * k * W_new * 4, 1.0, false));
    PO_TRY(ensure(h, w->d_wk_rl[nxt], (size_t)n_new * 8, 1.0, false));
    PO_TRY(walk_grow(h, w->d_wk_links, (size_t)links_used * sizeof(po::WkLink), (size_t)(links_used + n_new) * sizeof(po::WkLink)));
    hipEvent_t* ev = h->ev_lay + EV_WALK;
    HIP_TRY(h, hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(po::k_wk_advance, dim3(stride_grid(h, (uint64_t)n_new * k * W_new)), dim3(256), 0, st, n_new, C, k, P, w->wk_W, W_new,
                       rows.rows, h->ph_pbits, h->ph_fcand, h->ph_fext, h->ph_frl, w->d_wk_rows[nxt].as<uint32_t>(),
                       w->d_wk_links.as<po::WkLink>() + links_used, w->d_wk_rl[nxt].as<double>());
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(ev[1], st));
    PO_TRY(also());
    HIP_TRY(h, hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&S.ms_advance, ev[0], ev[1]);
    S.ms_total += S.ms_advance;
    // the state becomes the list
    if (w->wk_level_off.empty()) w->wk_level_off.push_back(0);
    w->wk_level_off.push_back(links_used + n_new);
    w->wk_cur = nxt;
    w->wk_n_cands = n_new;
    w->wk_W = W_new;
    return PO_OK;
}

po_status run_walk_step(po_handle* h, po_result* w, const po_phase_params& p, const po_phase_input& in, const uint32_t* b_reads, bool advance,
                        uint32_t* cand_out, uint32_t* ext_out, double* rl_out, uint64_t cap, uint64_t* n_out) {
    po_walk_stats& S = h->wkstats;
    S = po_walk_stats();
    const uint32_t k = p.ploidy, P = p.n_paths, C = p.n_cands, R = p.n_reads;
    const uint32_t n_block = (uint32_t)w->wk_reads.size();
    S.n_cands_in = S.n_cands_out = C;
    S.depth = walk_depth(w);
    S.n_block_reads = n_block;
    S.words_per_slot = w->wk_W;
    // the block-stable id of every b read: one merge of two ascending lists; the new ones are numbered in the order of b_reads
    std::vector<uint32_t> xl(p.n_b), fresh;
    {
        size_t at = 0;
        for (uint32_t j = 0; j < p.n_b; ++j) {
            while (at < w->wk_sorted.size() && w->wk_sorted[at].first < b_reads[j]) ++at;
            if (at < w->wk_sorted.size() && w->wk_sorted[at].first == b_reads[j]) {
                xl[j] = w->wk_sorted[at].second;
            } else {
                xl[j] = n_block + (uint32_t)fresh.size();
                fresh.push_back(b_reads[j]);
            }
        }
    }
    S.n_new_reads = fresh.size();
    if ((uint64_t)n_block + fresh.size() >= (1ull << 31)) return fail(h, PO_ERR_CAPACITY, "po_walk_step: more than 2^31 - 1 reads in one block");
    const uint32_t nb = n_block + (uint32_t)fresh.size();
    const uint32_t n_aln = R ? in.aln_off[R] : 0, n_pids = in.path_off[P];
    std::vector<uint32_t> aln_b(n_aln), path_ids(n_pids), no_sets((size_t)C * k + 1, 0u);
    for (uint32_t j = 0; j < n_aln; ++j) aln_b[j] = xl[in.aln_b[j]];          // (every local id is below n_b: phase_check)
    for (uint32_t j = 0; j < n_pids; ++j) path_ids[j] = xl[in.path_ids[j]];
    po_phase_params p2 = p;
    p2.n_b = nb;
    po_phase_input in2 = in;
    in2.aln_b = aln_b.data();
    in2.path_ids = path_ids.data();
    in2.set_off = no_sets.data();
    in2.set_ids = nullptr;
    uint64_t Pk = 1;
    for (uint32_t i = 0; i < k; ++i) Pk *= P;
    const WalkRows rows{w->d_wk_rows[w->wk_cur].as<uint32_t>(), w->wk_W, w->wk_W ? n_block : 0u};
    uint64_t n_final64 = 0;
    PO_TRY(run_phase(h, p2, in2, (uint32_t)Pk, cand_out, ext_out, rl_out, cap, nullptr, &n_final64, &rows));
    const po_phase_stats& F = h->phstats;
    S.ms_bits = F.ms_intervals;
    S.ms_total = F.ms_total;
    if (advance && n_final64) {
        PO_TRY(walk_take_over(h, w, rows, C, P, nb, (uint32_t)n_final64, [] { return PO_OK; }));
        const uint32_t n_new = (uint32_t)n_final64, W_new = w->wk_W;
        w->wk_route = 1;
        for (uint32_t g : fresh) w->wk_reads.push_back(g);
        if (!fresh.empty()) {
            std::vector<std::pair<uint32_t, uint32_t>> merged(w->wk_sorted.size() + fresh.size()), added(fresh.size());
            for (size_t j = 0; j < fresh.size(); ++j) added[j] = {fresh[j], n_block + (uint32_t)j};   // (ascending: b_reads is)
            std::merge(w->wk_sorted.begin(), w->wk_sorted.end(), added.begin(), added.end(), merged.begin());
            w->wk_sorted.swap(merged);
        }
        S.advanced = 1;
        S.n_cands_out = n_new;
        S.depth = walk_depth(w);
        S.n_block_reads = w->wk_reads.size();
        S.words_per_slot = W_new;
    }
    *n_out = n_final64;
    return PO_OK;
}

// prune(candidate_sets, 1.0) on the state's log_rl: every candidate at the early returns, else those equal to the greatest
po_status run_walk_best(po_handle* h, po_result* w, uint32_t* cands_out, uint64_t cap, uint64_t* n_out, double* max_rl_out) {
    const uint32_t n = w->wk_n_cands;
    double max_rl = -(double)INFINITY;
    auto everyone = [&] {
        for (uint64_t j = 0; j < std::min<uint64_t>(cap, n); ++j)
            if (cands_out) cands_out[j] = (uint32_t)j;
        *n_out = n;
        if (max_rl_out) *max_rl_out = max_rl;
        return PO_OK;
    };
    if (walk_depth(w) == 0) return everyone();   // (one candidate, log_rl = -inf: nothing lies on the device)
    hipStream_t st = h->stream;
    PO_TRY(ensure(h, h->d_scalars, 128));
    const size_t at_keep = 256, at_place = at_keep + (((size_t)n + 255) & ~size_t(255)), at_out = at_place + ((size_t)n + 1) * 4;
    PO_TRY(ensure(h, w->d_wk_tmp, at_out + ((size_t)n + 1) * 4, 1.0, false));
    char* tmp = w->d_wk_tmp.as<char>();
    unsigned long long* key_d = reinterpret_cast<unsigned long long*>(tmp);
    uint8_t* keep = reinterpret_cast<uint8_t*>(tmp + at_keep);
    uint32_t *place = reinterpret_cast<uint32_t*>(tmp + at_place), *out = reinterpret_cast<uint32_t*>(tmp + at_out);
    const double* rl = w->d_wk_rl[w->wk_cur].as<double>();
    HIP_TRY(h, hipMemsetAsync(key_d, 0, 8, st));
    hipLaunchKernelGGL(po::k_wk_max, dim3(stride_grid(h, n)), dim3(256), 0, st, n, rl, key_d);
    HIP_TRY(h, hipGetLastError());
    PO_TRY(land_outputs(h, {}, key_d, 1));
    const uint64_t key = h->pinned[16];
    if (!key) return fail(h, PO_ERR_HIP, "internal: the candidates of po_walk_best have no greatest log_rl");
    const uint64_t bits = (key >> 63) ? (key & 0x7FFFFFFFFFFFFFFFull) : ~key;
    std::memcpy(&max_rl, &bits, 8);
    if (n < 2 || max_rl == -(double)INFINITY) return everyone();
    hipLaunchKernelGGL(po::k_ph_survive, dim3(stride_grid(h, n)), dim3(256), 0, st, n, rl, max_rl, 0.0, keep);   // log10(1.0)
    HIP_TRY(h, hipGetLastError());
    PO_TRY(prefix_sum<uint8_t>(h, keep, n, place, &h->pinned[3]));
    HIP_TRY(h, hipStreamSynchronize(st));
    const uint64_t n_best = h->pinned[3];
    if (!n_best || n_best > n) return fail(h, PO_ERR_HIP, "internal: the tie set of po_walk_best does not add up");
    hipLaunchKernelGGL(po::k_wk_pick, dim3(stride_grid(h, n)), dim3(256), 0, st, n, (uint32_t)n_best, keep, place, out);
    HIP_TRY(h, hipGetLastError());
    PO_TRY(land_outputs(h, {{out, (size_t)std::min<uint64_t>(cap, n_best) * 4, cands_out}}, key_d, 1));
    *n_out = n_best;
    if (max_rl_out) *max_rl_out = max_rl;
    return PO_OK;
}

po_status run_walk_history(po_handle* h, po_result* w, const uint32_t* cands, uint32_t n, uint32_t* ext_out) {
    const uint32_t depth = walk_depth(w);
    if (!n || !depth) return PO_OK;
    hipStream_t st = h->stream;
    const size_t at_cands = (((size_t)depth + 1) * 8 + 255) & ~size_t(255), at_out = at_cands + ((((size_t)n + 1) * 4 + 255) & ~size_t(255));
    PO_TRY(ensure(h, w->d_wk_tmp, at_out + (size_t)n * depth * 4, 1.0, false));
    char* tmp = w->d_wk_tmp.as<char>();
    unsigned long long* off_d = reinterpret_cast<unsigned long long*>(tmp);
    uint32_t *cands_d = reinterpret_cast<uint32_t*>(tmp + at_cands), *out = reinterpret_cast<uint32_t*>(tmp + at_out);
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the level offsets go up as they are");
    HIP_TRY(h, hipMemcpyAsync(off_d, w->wk_level_off.data(), ((size_t)depth + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(cands_d, cands, (size_t)n * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(po::k_wk_trace, dim3(stride_grid(h, n)), dim3(256), 0, st, n, depth, off_d, w->d_wk_links.as<po::WkLink>(), cands_d, out);
    HIP_TRY(h, hipGetLastError());
    PO_TRY(land_outputs(h, {{out, (size_t)n * depth * 4, ext_out}}, off_d, 1));
    return PO_OK;
}

// the bit rows of the named candidates come home; their bits become global read ids on the host, ascending per set
po_status run_walk_read_sets(po_handle* h, po_result* w, const uint32_t* cands, uint32_t n, uint64_t* off_out, uint32_t* ids_out, uint64_t cap,
                             uint64_t* n_ids_out) {
    const uint32_t k = w->wk_k, W = walk_depth(w) ? w->wk_W : 0;
    const size_t row_bytes = (size_t)k * W * 4;
    uint64_t total = 0;
    if (off_out) off_out[0] = 0;
    const uint32_t* land = nullptr;
    if (n && row_bytes) {
        hipStream_t st = h->stream;
        PO_TRY(ensure_host(h, h->scratch_host, (size_t)n * row_bytes));
        const char* rows = w->d_wk_rows[w->wk_cur].as<char>();
        for (uint32_t q = 0; q < n; ++q)
            HIP_TRY(h, hipMemcpyAsync(static_cast<char*>(h->scratch_host.p) + (size_t)q * row_bytes, rows + (size_t)cands[q] * row_bytes, row_bytes,
                                      hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipStreamSynchronize(st));
        land = static_cast<const uint32_t*>(h->scratch_host.p);
    }
    if (w->wk_route == 2 && land && w->wk_reads.size() != w->rs_n_block) {
        // the resident route keeps stable id -> global id on the device: it comes home when a read set is asked for
        std::vector<uint32_t> home(w->rs_n_block);
        HIP_TRY(h, hipMemcpyAsync(home.data(), w->d_rs_global.p, (size_t)w->rs_n_block * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        land = static_cast<const uint32_t*>(h->scratch_host.p);
        w->wk_reads.swap(home);
    }
    std::vector<uint32_t> one;
    for (uint64_t s = 0; s < (uint64_t)n * k; ++s) {
        one.clear();
        for (uint32_t x = 0; land && x < W; ++x) {
            uint32_t word = land[s * W + x];
            while (word) {
                const uint32_t id = x * 32 + (uint32_t)__builtin_ctz(word);
                word &= word - 1;
                if (id < w->wk_reads.size()) one.push_back(w->wk_reads[id]);
            }
        }
        std::sort(one.begin(), one.end());
        for (uint32_t g : one) {
            if (ids_out && total < cap) ids_out[total] = g;
            ++total;
        }
        if (off_out) off_out[s + 1] = total;
    }
    *n_ids_out = total;
    return PO_OK;
}

// ---- the alignment index and the relevant reads of a bubble (po_phase_index, po_phase_relevant, relevant.hip.h) ---------------

po_status run_phase_index(po_handle* h, po_result* rows, po_result* r) {
    const char* const name = "po_phase_index";
    hipStream_t st = h->stream;
    po_phase_index_stats& S = h->pxstats;
    S = po_phase_index_stats();
    const uint32_t n_ids = (uint32_t)h->len.size(), n_rows = (uint32_t)rows->count;   // (2 * rows < 2^31: the entry point)
    S.n_rows = n_rows;
    r->special = 1;
    r->elem = 1;
    r->ix_n_ids = n_ids;
    const uint32_t n_slots = po::rr_table_slots(n_rows);
    r->ix_n_slots = n_slots;
    PO_TRY(lay_events(h));
    hipEvent_t* ev = h->ev_lay + EV_PHASE_INDEX;
    PO_TRY(rows_to_device(h, rows));
    DevBuf* B = h->d_rr;
    const size_t nn = (size_t)n_ids + 2;
    PO_TRY(ensure(h, h->d_scalars, 128));
    PO_TRY(ensure(h, B[XB_CNT], 128));
    for (int k : {XB_DEG, XB_CUR}) PO_TRY(ensure(h, B[k], nn * 4));
    // (what leaves the handle with the result is not carved out of the handle's arena)
    PO_TRY(ensure(h, r->d_ixtable, (size_t)n_slots * 8, 1.0, false));
    PO_TRY(ensure(h, r->d_ixval, (size_t)n_slots * 4, 1.0, false));
    PO_TRY(ensure(h, r->d_ixoff, nn * 4, 1.0, false));
    PO_TRY(ensure(h, r->d_ixlen, nn * 4, 1.0, false));
    unsigned long long *cnt = B[XB_CNT].as<unsigned long long>(), *table = r->d_ixtable.as<unsigned long long>();
    uint32_t *deg = B[XB_DEG].as<uint32_t>(), *cur = B[XB_CUR].as<uint32_t>(), *tval = r->d_ixval.as<uint32_t>(),
             *off = r->d_ixoff.as<uint32_t>(), *d_len = r->d_ixlen.as<uint32_t>();
    const po::Row* d_rows = rows->d_rows.as<po::Row>();
    HIP_TRY(h, hipEventRecord(ev[0], st));
    HIP_TRY(h, hipMemsetAsync(cnt, 0, 128, st));
    for (uint32_t* p : {deg, cur, off}) HIP_TRY(h, hipMemsetAsync(p, 0, nn * 4, st));
    HIP_TRY(h, hipMemsetAsync(table, 0xFF, (size_t)n_slots * 8, st));
    HIP_TRY(h, hipMemsetAsync(tval, 0, (size_t)n_slots * 4, st));
    if (n_ids) HIP_TRY(h, hipMemcpyAsync(d_len, h->len.data(), (size_t)n_ids * 4, hipMemcpyHostToDevice, st));
    if (n_rows) hipLaunchKernelGGL(po::k_rr_insert, dim3(stride_grid(h, n_rows)), dim3(256), 0, st, d_rows, n_rows, n_ids, table, tval, n_slots, deg, cnt);
    if (n_ids) hipLaunchKernelGGL(po::k_rr_degree, dim3(stride_grid(h, n_ids)), dim3(256), 0, st, deg, n_ids, cnt);
    HIP_TRY(h, hipGetLastError());
    PO_TRY(prefix_sum<uint32_t>(h, deg, n_ids, off, &h->pinned[2]));   // (off[n_ids] is the closing sentinel: the number of keys)
    HIP_TRY(h, hipMemcpyAsync(h->pinned + 16, cnt, po::RX_N * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipEventRecord(ev[1], st));
    HIP_TRY(h, hipStreamSynchronize(st));
    S.n_invalid = h->pinned[16 + po::RX_INVALID];
    S.n_keys = h->pinned[16 + po::RX_KEYS];
    S.max_degree = h->pinned[16 + po::RX_MAXDEG];
    if (S.n_invalid) return fail(h, PO_ERR_INVALID, std::string(name) + ": a row names a read the handle does not hold");
    if (h->pinned[2] != S.n_keys || S.n_keys > 2ull * n_rows)
        return fail(h, PO_ERR_HIP, std::string("internal: the segments of ") + name + " do not add up");
    const uint32_t n_keys = (uint32_t)S.n_keys;
    r->ix_n_keys = n_keys;
    PO_TRY(ensure(h, r->d_ixent, ((size_t)n_keys + 1) * sizeof(po::RrEntry), 1.0, false));
    PO_TRY(ensure(h, B[XB_TMP], ((size_t)n_keys + 1) * sizeof(po::RrEntry)));
    PO_TRY(ensure(h, B[XB_EX], ((size_t)n_keys + 1) * 4));
    po::RrEntry *tmp = B[XB_TMP].as<po::RrEntry>(), *entries = r->d_ixent.as<po::RrEntry>();
    uint32_t* ex = B[XB_EX].as<uint32_t>();
    if (n_keys) {
        hipLaunchKernelGGL(po::k_rr_fill, dim3(stride_grid(h, n_slots)), dim3(256), 0, st, table, tval, n_slots, d_rows, n_rows, n_ids, off, cur, tmp,
                           ex, n_keys);
        hipLaunchKernelGGL(po::k_rr_sort, dim3(stride_grid(h, n_keys)), dim3(256), 0, st, tmp, ex, off, n_keys, n_ids, entries);
    }
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(ev[2], st));
    if (n_keys) hipLaunchKernelGGL(po::k_rr_place, dim3(stride_grid(h, n_keys)), dim3(256), 0, st, entries, ex, n_keys, table, tval, n_slots);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(ev[3], st));
    HIP_TRY(h, hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&S.ms_insert, ev[0], ev[1]);
    (void)hipEventElapsedTime(&S.ms_fill, ev[1], ev[2]);
    (void)hipEventElapsedTime(&S.ms_place, ev[2], ev[3]);
    (void)hipEventElapsedTime(&S.ms_total, ev[0], ev[3]);
    return PO_OK;
}

// The checks of po_phase_relevant in front of the device, in the order the header lists them: the sentence of the first one
// that fails, empty when the call may go on.
std::string relevant_check(const po_handle* h, const po_result* index, const po_relevant_params* p, const po_relevant_input* in,
                           const char* who = "po_phase_relevant") {
    const std::string name = std::string(who) + ": ";
    if (!p || !in) return name + "no parameters";
    if (p->reserved || p->reserved2) return name + "bad parameters";
    if (p->mode > 1) return name + "the mode must be 0 (spanning) or 1 (all)";
    if ((!in->cur_graph && in->n_cur_graph) || (!in->prev_graph && in->n_prev_graph) || (!in->prev_aligning && in->n_prev_aligning) ||
        ((!in->pred_read || !in->pred_edge_len) && in->n_pred))
        return name + "a list is missing";
    const uint64_t n_ids = h->len.size();
    if (in->n_cur_graph + in->n_prev_graph + in->n_prev_aligning + in->n_pred >= (1ull << 31)) return name + "the lists are too long for one call";
    for (const auto& l : {std::make_pair(in->cur_graph, in->n_cur_graph), std::make_pair(in->prev_graph, in->n_prev_graph),
                          std::make_pair(in->prev_aligning, in->n_prev_aligning), std::make_pair(in->pred_read, in->n_pred)})
        for (uint64_t i = 0; i < l.second; ++i)
            if (l.first[i] >= n_ids) return name + "a list names a read the handle does not hold";
    if (index->h != h) return name + "the index belongs to another handle";
    if (index->special != 1) return name + "needs the result of po_phase_index";
    if (index->ix_n_ids != n_ids) return name + "reads were added to the handle after the index was built";
    return std::string();
}

// What the next device call on a walk's resident state does first: the two bitsets and stable_of exist for the handle's read
// ids (prev_graph, then prev_aligning, W + 1 words each; stable_of all RS_NONE), and what a reset left to clear is cleared --
// the map over the old block's reads alone, so a reset costs the block and not the read set.
po_status rs_prepare(po_handle* h, po_result* w) {
    hipStream_t st = h->stream;
    const uint32_t n_ids = (uint32_t)h->len.size();
    const size_t Wp = (size_t)cdiv(n_ids, 32) + 1;
    if (!w->d_rs_prev.p || w->rs_n_ids != n_ids) {
        if (w->d_rs_prev.p && (w->rs_live || w->rs_n_block || w->wk_route == 2))
            return fail(h, PO_ERR_INVALID, "po_walk_relevant: reads were added to the handle inside a block of the walk");
        PO_TRY(ensure(h, w->d_rs_prev, 2 * Wp * 4, 1.0, false));
        PO_TRY(ensure(h, w->d_rs_stable, ((size_t)n_ids + 1) * 4, 1.0, false));
        HIP_TRY(h, hipMemsetAsync(w->d_rs_prev.p, 0, 2 * Wp * 4, st));
        HIP_TRY(h, hipMemsetAsync(w->d_rs_stable.p, 0xFF, ((size_t)n_ids + 1) * 4, st));   // (RS_NONE)
        w->rs_n_ids = n_ids;
        w->rs_unmap_n = 0;
        w->rs_clear_prev = false;
        return PO_OK;
    }
    if (w->rs_unmap_n) {
        hipLaunchKernelGGL(po::k_rs_unmap, dim3(stride_grid(h, w->rs_unmap_n)), dim3(256), 0, st, w->rs_unmap_n, w->d_rs_global.as<uint32_t>(), n_ids,
                           w->d_rs_stable.as<uint32_t>());
        HIP_TRY(h, hipGetLastError());
        w->rs_unmap_n = 0;
    }
    if (w->rs_clear_prev) {
        HIP_TRY(h, hipMemsetAsync(w->d_rs_prev.p, 0, 2 * Wp * 4, st));
        w->rs_clear_prev = false;
    }
    return PO_OK;
}

// `walk` (po_walk_relevant): the gather works in the walk's own buffers and leaves its arrays there; prev_aligning and --
// unless `no_prev_graph` -- prev_graph are the walk's bitsets, and nothing but the sizes comes home.
po_status run_relevant(po_handle* h, const po_result* index, const po_relevant_params& p, const po_relevant_input& in, po_result* r,
                       po_result* walk = nullptr, bool no_prev_graph = false) {
    const char* const name = walk ? "po_walk_relevant" : "po_phase_relevant";
    hipStream_t st = h->stream;
    po_relevant_stats& S = h->rvstats;
    S = po_relevant_stats();
    r->special = 2;
    r->elem = 1;
    r->rv = po_relevant_dims();
    const uint32_t n_cur = (uint32_t)in.n_cur_graph, n_pg = (uint32_t)in.n_prev_graph, n_pa = (uint32_t)in.n_prev_aligning,
                   n_pred = (uint32_t)in.n_pred;
    if (walk) {
        // the walk's buffers are about to be written: the gather that lived there is stale from here on
        if (walk->rs_live) {
            walk->rs_live->rv_stale = true;
            walk->rs_live->rv_walk = nullptr;
            walk->rs_live = nullptr;
        }
        r->rv_resident = true;
        r->rv_mode = p.mode;
        r->rv_depth = walk->wk_level_off.empty() ? 0u : (uint32_t)(walk->wk_level_off.size() - 1);
        r->rv_empty = !n_cur;
        if (n_cur) PO_TRY(rs_prepare(h, walk));
        r->rv_walk = walk;
        walk->rs_live = r;
    }
    if (!n_cur) return PO_OK;   // (every size 0)
    const uint32_t n_ids = index->ix_n_ids, n_keys = index->ix_n_keys, n_slots = index->ix_n_slots, W = cdiv(n_ids, 32);
    PO_TRY(lay_events(h));
    hipEvent_t* ev = h->ev_lay + EV_RELEVANT;
    DevBuf* B = walk ? walk->d_rs_rel : h->d_rr;
    const bool arena = !walk;   // (what belongs to a result is not carved out of the handle's arena)
    // the five lists behind one another, as one upload
    const size_t n_lists = (size_t)n_cur + n_pg + n_pa + 2 * (size_t)n_pred;
    std::vector<uint32_t> lists(n_lists);
    {
        uint32_t* at = lists.data();
        for (const auto& l : {std::make_pair((const void*)in.cur_graph, n_cur), std::make_pair((const void*)in.prev_graph, n_pg),
                              std::make_pair((const void*)in.prev_aligning, n_pa), std::make_pair((const void*)in.pred_read, n_pred),
                              std::make_pair((const void*)in.pred_edge_len, n_pred)}) {
            if (l.second) std::memcpy(at, l.first, (size_t)l.second * 4);
            at += l.second;
        }
    }
    const size_t Wp = (size_t)W + 1;   // (a scan writes a closing sentinel)
    PO_TRY(ensure(h, h->d_scalars, 128));
    PO_TRY(ensure(h, B[XB_CNT], 128, 1.0, arena));
    PO_TRY(ensure(h, B[XB_LISTS], n_lists * 4, 1.0, arena));
    PO_TRY(ensure(h, B[XB_BITS], 6 * Wp * 4, 1.0, arena));
    PO_TRY(ensure(h, B[XB_WCNT], 3 * Wp * 4, 1.0, arena));
    PO_TRY(ensure(h, B[XB_WRANK], 3 * Wp * 4, 1.0, arena));
    unsigned long long* cnt = B[XB_CNT].as<unsigned long long>();
    uint32_t* d_lists = B[XB_LISTS].as<uint32_t>();
    const uint32_t *d_cur = d_lists, *d_pg = d_cur + n_cur, *d_pa = d_pg + n_pg, *d_pred = d_pa + n_pa;
    const int32_t* d_plen = reinterpret_cast<const int32_t*>(d_pred + n_pred);
    uint32_t* bits = B[XB_BITS].as<uint32_t>();
    uint32_t *ca = bits, *gc = bits + 2 * Wp, *rel = bits + 4 * Wp, *g = bits + 5 * Wp;
    uint32_t *pa = walk ? walk->d_rs_prev.as<uint32_t>() + Wp : bits + Wp, *gp = walk ? walk->d_rs_prev.as<uint32_t>() : bits + 3 * Wp;
    uint32_t *wcnt = B[XB_WCNT].as<uint32_t>(), *wrank = B[XB_WRANK].as<uint32_t>();
    const uint32_t* off = index->d_ixoff.as<uint32_t>();
    const po::RrEntry* entries = index->d_ixent.as<po::RrEntry>();
    const uint32_t cap = (uint32_t)h->n_cu * 8, word_grid = stride_grid(h, W);
    auto wave_grid = [&](uint32_t n) { return std::max<uint32_t>(1u, std::min<uint32_t>(cdiv(n, 4), cap)); };   // one wave per item, four to a workgroup
    HIP_TRY(h, hipEventRecord(ev[0], st));
    HIP_TRY(h, hipMemsetAsync(cnt, 0, 128, st));
    HIP_TRY(h, hipMemsetAsync(bits, 0, 4 * Wp * 4, st));
    HIP_TRY(h, hipMemcpyAsync(d_lists, lists.data(), n_lists * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(po::k_rr_mark, dim3(stride_grid(h, n_cur)), dim3(256), 0, st, d_cur, n_cur, n_ids, ca);
    hipLaunchKernelGGL(po::k_rr_mark, dim3(stride_grid(h, n_cur)), dim3(256), 0, st, d_cur, n_cur, n_ids, gc);
    if (n_pg) hipLaunchKernelGGL(po::k_rr_mark, dim3(stride_grid(h, n_pg)), dim3(256), 0, st, d_pg, n_pg, n_ids, gp);
    if (n_pa) hipLaunchKernelGGL(po::k_rr_mark, dim3(stride_grid(h, n_pa)), dim3(256), 0, st, d_pa, n_pa, n_ids, pa);
    hipLaunchKernelGGL(po::k_rr_mark_seg, dim3(wave_grid(n_cur)), dim3(256), 0, st, d_cur, n_cur, n_ids, off, entries, n_keys, ca);
    hipLaunchKernelGGL(po::k_rr_count, dim3(word_grid), dim3(256), 0, st, ca, pa, W, cnt);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(h->pinned + 16, cnt, po::RG_N * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipEventRecord(ev[1], st));
    HIP_TRY(h, hipStreamSynchronize(st));   // (the lists are on the device: `lists` may go)
    const uint64_t n_ca = h->pinned[16 + po::RG_CA], n_span = h->pinned[16 + po::RG_SPAN];
    if (n_ca > n_ids || n_span > n_ca) return fail(h, PO_ERR_HIP, std::string("internal: the aligning reads of ") + name + " do not add up");
    const bool fell_back = p.mode == 0 && n_span < p.min_spanning_reads, use_pa = p.mode == 0 && !fell_back;
    const bool use_prev = !fell_back && !no_prev_graph;
    // (the walk knows how many reads prev_graph holds at the most: that bounds G as n_prev_graph does)
    const uint32_t n_rel = (uint32_t)(use_pa ? n_span : n_ca), g_room = !use_prev ? n_cur : n_cur + (walk ? walk->rs_prevg_bound : n_pg);
    PO_TRY(ensure(h, B[XB_CA], (n_ca + 1) * 4, 1.0, arena));
    PO_TRY(ensure(h, B[XB_REL], ((size_t)n_rel + 1) * 4, 1.0, arena));
    PO_TRY(ensure(h, B[XB_B], ((size_t)g_room + 1) * 4, 1.0, arena));
    for (int k : {XB_ALNCNT, XB_ALNOFF, XB_OM}) PO_TRY(ensure(h, B[k], ((size_t)n_rel + 2) * 4, 1.0, arena));
    uint32_t *l_ca = B[XB_CA].as<uint32_t>(), *l_rel = B[XB_REL].as<uint32_t>(), *l_b = B[XB_B].as<uint32_t>(),
             *aln_cnt = B[XB_ALNCNT].as<uint32_t>(), *aln_off = B[XB_ALNOFF].as<uint32_t>();
    int32_t* om = B[XB_OM].as<int32_t>();
    HIP_TRY(h, hipMemsetAsync(aln_off, 0, ((size_t)n_rel + 2) * 4, st));   // (no relevant read: the scan writes nothing)
    hipLaunchKernelGGL(po::k_rr_select, dim3(word_grid), dim3(256), 0, st, ca, pa, gc, gp, W, (uint32_t)use_pa, (uint32_t)use_prev, rel, g, wcnt,
                       wcnt + Wp, wcnt + 2 * Wp);
    HIP_TRY(h, hipGetLastError());
    for (int k = 0; k < 3; ++k) PO_TRY(prefix_sum<uint32_t>(h, wcnt + k * Wp, W, wrank + k * Wp, &h->pinned[2 + k]));
    hipLaunchKernelGGL(po::k_rr_list, dim3(word_grid), dim3(256), 0, st, ca, wrank, W, l_ca, (uint32_t)n_ca);
    hipLaunchKernelGGL(po::k_rr_list, dim3(word_grid), dim3(256), 0, st, rel, wrank + Wp, W, l_rel, n_rel);
    hipLaunchKernelGGL(po::k_rr_list, dim3(word_grid), dim3(256), 0, st, g, wrank + 2 * Wp, W, l_b, g_room);
    HIP_TRY(h, hipEventRecord(ev[2], st));
    if (n_rel) {
        hipLaunchKernelGGL(po::k_rr_alncount, dim3(wave_grid(n_rel)), dim3(256), 0, st, l_rel, n_rel, n_ids, off, entries, n_keys, g, aln_cnt);
        hipLaunchKernelGGL(po::k_rr_omax, dim3(stride_grid(h, n_rel)), dim3(256), 0, st, l_rel, n_rel, n_ids, index->d_ixlen.as<uint32_t>(), d_pred,
                           d_plen, n_pred, index->d_ixtable.as<unsigned long long>(), index->d_ixval.as<uint32_t>(), n_slots, entries, n_keys,
                           om);
    }
    HIP_TRY(h, hipGetLastError());
    PO_TRY(prefix_sum<uint32_t>(h, aln_cnt, n_rel, aln_off, &h->pinned[5]));
    HIP_TRY(h, hipStreamSynchronize(st));
    const uint64_t n_b = h->pinned[4], n_aln = h->pinned[5];
    if (h->pinned[2] != n_ca || h->pinned[3] != n_rel || n_b > g_room || n_aln > n_keys)
        return fail(h, PO_ERR_HIP, std::string("internal: the lists of ") + name + " do not add up");
    for (int k : {XB_ALNB, XB_A0, XB_A1}) PO_TRY(ensure(h, B[k], (n_aln + 1) * 4, 1.0, arena));
    uint32_t* aln_b = B[XB_ALNB].as<uint32_t>();
    int32_t *a0 = B[XB_A0].as<int32_t>(), *a1 = B[XB_A1].as<int32_t>();
    if (n_aln)
        hipLaunchKernelGGL(po::k_rr_alnwrite, dim3(wave_grid(n_rel)), dim3(256), 0, st, l_rel, n_rel, n_ids, off, entries, n_keys, g, wrank + 2 * Wp,
                           aln_off, (uint32_t)n_aln, aln_b, a0, a1);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(ev[3], st));
    r->rv.n_cur_aligning = S.n_cur_aligning = n_ca;
    r->rv.n_spanning = S.n_spanning = n_span;
    r->rv.n_relevant = S.n_relevant = n_rel;
    r->rv.n_alignments = S.n_alignments = n_aln;
    r->rv.n_b = S.n_b = n_b;
    r->rv.fell_back = S.fell_back = fell_back;
    if (walk) {
        // the arrays stay where they are; the last launches are not waited for, so their time is not in the figures
        r->rv_used_prev = use_prev;
        (void)hipEventElapsedTime(&S.ms_mark, ev[0], ev[1]);
        (void)hipEventElapsedTime(&S.ms_lists, ev[1], ev[2]);
        S.ms_total = S.ms_mark + S.ms_lists;
        return PO_OK;
    }
    r->rv_ca.resize(n_ca);
    r->rv_rel.resize(n_rel);
    r->rv_om.resize(n_rel);
    r->rv_alnoff.resize((size_t)n_rel + 1);
    r->rv_alnb.resize(n_aln);
    r->rv_a0.resize(n_aln);
    r->rv_a1.resize(n_aln);
    r->rv_b.resize(n_b);
    PO_TRY(land_outputs(h, {{l_ca, n_ca * 4, r->rv_ca.data()}, {l_rel, (size_t)n_rel * 4, r->rv_rel.data()}, {om, (size_t)n_rel * 4, r->rv_om.data()},
                            {aln_off, ((size_t)n_rel + 1) * 4, r->rv_alnoff.data()}, {aln_b, n_aln * 4, r->rv_alnb.data()},
                            {a0, n_aln * 4, r->rv_a0.data()}, {a1, n_aln * 4, r->rv_a1.data()}, {l_b, n_b * 4, r->rv_b.data()}}, cnt, po::RG_N));
    (void)hipEventElapsedTime(&S.ms_mark, ev[0], ev[1]);
    (void)hipEventElapsedTime(&S.ms_lists, ev[1], ev[2]);
    (void)hipEventElapsedTime(&S.ms_alignments, ev[2], ev[3]);
    (void)hipEventElapsedTime(&S.ms_total, ev[0], ev[3]);
    return PO_OK;
}

// ---- the resident route through one step of the walk (po_walk_relevant, po_walk_step_resident, resident.hip.h) -------------

// is `rel` the live gather of walk `w`?  The sentence, empty when it is.
std::string gather_live(const po_result* w, const po_result* rel, const char* who) {
    const std::string name = std::string(who) + ": ";
    if (rel->rv_stale || !rel->rv_walk)
        return name + "the gather is stale: a later po_walk_relevant, a po_walk_reset or the freeing of its walk has taken its arrays";
    if (w && rel->rv_walk != w) return name + "the gather belongs to another walk";
    if (rel->rv_walk->rs_live != rel) return name + "the gather is stale: a later po_walk_relevant, a po_walk_reset or the freeing of its walk has taken its arrays";
    return std::string();
}

// The checks of po_walk_step_resident in front of the device, in the order the header lists them.
std::string resident_check(const po_handle* h, const po_result* w, const po_result* rel, const po_phase_params& p, const po_phase_input& in,
                           uint64_t& Pk) {
    const std::string name = "po_walk_step_resident: ";
    if (w->special != WALK_KIND) return name + "needs the result of po_walk_create";
    if (w->h != h) return name + "the walk belongs to another handle";
    if (rel->special != 2 || !rel->rv_resident) return name + "needs the result of po_walk_relevant";
    if (rel->h != h) return name + "the gather belongs to another handle";
    const std::string stale = gather_live(w, rel, "po_walk_step_resident");
    if (!stale.empty()) return stale;
    if (in.overlap_max || in.aln_off || in.aln_b || in.aln_a0 || in.aln_a1 || in.set_off || in.set_ids)
        return name + "only path_off, path_ids and levels are given: every other array must be NULL, it is the gather's or the walk's";
    if (p.reserved || p.reserved2 || !(p.threshold >= 0.0) || p.n_levels > po::PH_MAX_LEVELS) return name + "bad parameters";
    if (p.n_reads != rel->rv.n_relevant) return name + "n_reads is not the number of relevant reads of the gather";
    if (p.n_b != rel->rv.n_b) return name + "n_b is not the number of b reads of the gather";
    if (p.ploidy != w->wk_k) return name + "the ploidy is not the walk's";
    if (p.n_cands != w->wk_n_cands) return name + "n_cands is not the number of candidates the walk holds";
    if ((p.start_of_block != 0) != (walk_depth(w) == 0)) return name + "start_of_block is not the walk's";
    if (rel->rv_depth != walk_depth(w)) return name + "the gather was made at another depth of the walk";
    if (w->wk_route == 1) return name + "the block advanced by po_walk_step: the two routes do not mix before po_walk_reset";
    if (p.n_paths < 1 || p.n_paths > po::PH_MAX_P) return name + "the number of paths must be 1 to 64";
    Pk = 1;
    for (uint32_t i = 0; i < p.ploidy; ++i) Pk *= p.n_paths;
    if (Pk >= (1ull << 31) || Pk * p.n_cands >= (1ull << 31)) return name + "too many extensions for one call";
    if (!in.path_off || (p.prune && p.n_levels && !in.levels)) return name + "an input array is missing";
    if (!phase_offsets_ok(in.path_off, p.n_paths)) return name + "the offsets of the paths do not start at 0 or decrease";
    const uint32_t n_pids = in.path_off[p.n_paths];
    if (n_pids && !in.path_ids) return name + "an input array is missing";
    const uint64_t n_ids = h->len.size();
    for (uint32_t j = 0; j < n_pids; ++j)
        if (in.path_ids[j] >= n_ids) return name + "a path names a read the handle does not hold";
    return std::string();
}

enum { RS_FLAG, RS_RANK, RS_XL, RS_ALNB, RS_PIN, RS_PIDS, RS_N };

po_status run_walk_step_resident(po_handle* h, po_result* w, po_result* rel, const po_phase_params& p, const po_phase_input& in, bool advance,
                                 uint32_t* cand_out, uint32_t* ext_out, double* rl_out, uint64_t cap, uint64_t* n_out) {
    static_assert(RS_N == sizeof(po_result::d_rs_step) / sizeof(DevBuf), "the scratch of the resident step");
    hipStream_t st = h->stream;
    po_walk_stats& S = h->wkstats;
    S = po_walk_stats();
    const uint32_t k = p.ploidy, P = p.n_paths, C = p.n_cands;
    S.n_cands_in = S.n_cands_out = C;
    S.depth = walk_depth(w);
    S.words_per_slot = w->wk_W;
    PO_TRY(rs_prepare(h, w));   // (what a reset left to clear, before anything reads the map)
    const uint32_t n_block = w->rs_n_block, n_ids = w->rs_n_ids, n_b = (uint32_t)rel->rv.n_b, n_aln = (uint32_t)rel->rv.n_alignments;
    const uint32_t n_pids = in.path_off[P];
    const size_t Wp = (size_t)cdiv(n_ids, 32) + 1;
    S.n_block_reads = n_block;
    DevBuf *G = w->d_rs_rel, *T = w->d_rs_step;
    PO_TRY(ensure(h, h->d_scalars, 128));
    for (int b : {RS_FLAG, RS_XL}) PO_TRY(ensure(h, T[b], ((size_t)n_b + 1) * 4, 1.0, false));
    PO_TRY(ensure(h, T[RS_RANK], ((size_t)n_b + 2) * 4, 1.0, false));
    PO_TRY(ensure(h, T[RS_ALNB], ((size_t)n_aln + 1) * 4, 1.0, false));
    for (int b : {RS_PIN, RS_PIDS}) PO_TRY(ensure(h, T[b], ((size_t)n_pids + 1) * 4, 1.0, false));
    uint32_t *flag = T[RS_FLAG].as<uint32_t>(), *rank = T[RS_RANK].as<uint32_t>(), *xl = T[RS_XL].as<uint32_t>(), *alnb = T[RS_ALNB].as<uint32_t>(),
             *pin = T[RS_PIN].as<uint32_t>(), *pids = T[RS_PIDS].as<uint32_t>();
    uint32_t *stable_of = w->d_rs_stable.as<uint32_t>();
    const uint32_t* b_reads = G[XB_B].as<uint32_t>();
    PO_TRY(lay_events(h));
    hipEvent_t* ev = h->ev_lay + EV_RESIDENT;   // (0..1 the flags and their scan, 2..3 the translation, 4 behind the commit)
    if (n_pids) HIP_TRY(h, hipMemcpyAsync(pin, in.path_ids, (size_t)n_pids * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipEventRecord(ev[0], st));
    // the reads of b_reads that are new to the block, numbered in the order of b_reads; the one count the host needs: W
    uint64_t n_fresh = 0;
    if (n_b) {
        hipLaunchKernelGGL(po::k_rs_flag, dim3(stride_grid(h, n_b)), dim3(256), 0, st, n_b, b_reads, n_ids, stable_of, flag);
        HIP_TRY(h, hipGetLastError());
        PO_TRY(prefix_sum<uint32_t>(h, flag, n_b, rank, &h->pinned[2]));
        HIP_TRY(h, hipEventRecord(ev[1], st));
        HIP_TRY(h, hipStreamSynchronize(st));   // (the path ids are on the device too: the caller's array may go)
        n_fresh = h->pinned[2];
        if (n_fresh > n_b) return fail(h, PO_ERR_HIP, "internal: the new reads of po_walk_step_resident do not add up");
    } else {
        HIP_TRY(h, hipEventRecord(ev[1], st));
        if (n_pids) HIP_TRY(h, hipStreamSynchronize(st));
    }
    S.n_new_reads = n_fresh;
    if ((uint64_t)n_block + n_fresh >= (1ull << 31)) return fail(h, PO_ERR_CAPACITY, "po_walk_step_resident: more than 2^31 - 1 reads in one block");
    const uint32_t nb = n_block + (uint32_t)n_fresh;
    HIP_TRY(h, hipEventRecord(ev[2], st));
    if (n_b) {
        hipLaunchKernelGGL(po::k_rs_local, dim3(stride_grid(h, n_b)), dim3(256), 0, st, n_b, b_reads, n_ids, stable_of, n_block, flag, rank, xl);
        if (n_aln) hipLaunchKernelGGL(po::k_rs_alnb, dim3(stride_grid(h, n_aln)), dim3(256), 0, st, n_aln, G[XB_ALNB].as<uint32_t>(), n_b, xl, alnb);
    }
    if (n_pids) {
        if (n_b)
            hipLaunchKernelGGL(po::k_rs_paths, dim3(stride_grid(h, n_pids)), dim3(256), 0, st, n_pids, pin, n_ids, G[XB_BITS].as<uint32_t>() + 5 * Wp,
                               G[XB_WRANK].as<uint32_t>() + 2 * Wp, n_b, xl, pids);
        else
            HIP_TRY(h, hipMemsetAsync(pids, 0xFF, (size_t)n_pids * 4, st));   // (no b read: every path read is outside, RS_NONE)
    }
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(ev[3], st));
    po_phase_params p2 = p;
    p2.n_b = nb;
    std::vector<uint32_t> no_sets((size_t)C * k + 1, 0u);
    po_phase_input in2 = in;
    in2.set_off = no_sets.data();
    uint64_t Pk = 1;
    for (uint32_t i = 0; i < k; ++i) Pk *= P;
    const WalkRows rows{w->d_wk_rows[w->wk_cur].as<uint32_t>(), w->wk_W, w->wk_W ? n_block : 0u};
    const PhaseDev dev{G[XB_OM].as<int32_t>(), G[XB_ALNOFF].as<uint32_t>(), alnb, G[XB_A0].as<int32_t>(), G[XB_A1].as<int32_t>(), pids, n_aln, n_pids};
    uint64_t n_final64 = 0;
    PO_TRY(run_phase(h, p2, in2, (uint32_t)Pk, cand_out, ext_out, rl_out, cap, nullptr, &n_final64, &rows, &dev));
    const po_phase_stats& F = h->phstats;
    S.ms_bits = F.ms_intervals;
    S.ms_total = F.ms_total;
    {   // (the synchronises of run_phase lie behind the four events)
        float a = 0.f, b = 0.f;
        (void)hipEventElapsedTime(&a, ev[0], ev[1]);
        (void)hipEventElapsedTime(&b, ev[2], ev[3]);
        S.ms_resident = a + b;
        S.ms_total += S.ms_resident;
    }
    if (advance && n_final64) {
        PO_TRY(walk_grow(h, w->d_rs_global, (size_t)n_block * 4, ((size_t)nb + 1) * 4));
        PO_TRY(walk_take_over(h, w, rows, C, P, nb, (uint32_t)n_final64, [&]() -> po_status {
            // the map and the two sets follow the candidates, in front of the same synchronise
            if (n_fresh)
                hipLaunchKernelGGL(po::k_rs_commit, dim3(stride_grid(h, n_b)), dim3(256), 0, st, n_b, b_reads, n_ids, flag, xl, nb, stable_of,
                                   w->d_rs_global.as<uint32_t>());
            if (!rel->rv_empty) {
                uint32_t *bits = G[XB_BITS].as<uint32_t>(), *prev = w->d_rs_prev.as<uint32_t>();
                hipLaunchKernelGGL(po::k_rs_or, dim3(stride_grid(h, Wp - 1)), dim3(256), 0, st, (uint32_t)(Wp - 1), bits + 2 * Wp, bits, prev, prev + Wp);
            }
            HIP_TRY(h, hipGetLastError());
            HIP_TRY(h, hipEventRecord(ev[4], st));
            return PO_OK;
        }));
        {
            float c = 0.f;
            (void)hipEventElapsedTime(&c, (h->ev_lay + EV_WALK)[1], ev[4]);
            S.ms_resident += c;
            S.ms_total += c;
        }
        w->wk_route = 2;
        w->rs_n_block = nb;
        w->wk_reads.clear();   // (the host copy of global_of, fetched when po_walk_read_sets asks)
        w->rs_prevg_bound = rel->rv_used_prev ? n_b : (uint32_t)std::min<uint64_t>(n_ids, (uint64_t)w->rs_prevg_bound + n_b);
        S.advanced = 1;
        S.n_cands_out = n_final64;
        S.depth = walk_depth(w);
        S.n_block_reads = nb;
        S.words_per_slot = w->wk_W;
    }
    *n_out = n_final64;
    return PO_OK;
}

// one of the walk's two sets as an ascending list: the set bits of every word, the library's prefix sum, k_rr_list
po_status run_walk_prev_copy(po_handle* h, po_result* w, uint32_t which, uint32_t* ids_out, uint64_t cap, uint64_t* n_out) {
    hipStream_t st = h->stream;
    const uint32_t W = cdiv(w->rs_n_ids, 32);
    const size_t Wp = (size_t)W + 1;
    if (!W) return PO_OK;
    PO_TRY(ensure(h, h->d_scalars, 128));
    PO_TRY(ensure(h, w->d_wk_tmp, 2 * Wp * 4 + 256, 1.0, false));
    uint32_t *cnt = w->d_wk_tmp.as<uint32_t>(), *rank = cnt + Wp;
    const uint32_t* bits = w->d_rs_prev.as<uint32_t>() + (which ? Wp : 0);
    hipLaunchKernelGGL(po::k_rs_popc, dim3(stride_grid(h, W)), dim3(256), 0, st, W, bits, cnt);
    HIP_TRY(h, hipGetLastError());
    PO_TRY(prefix_sum<uint32_t>(h, cnt, W, rank, &h->pinned[2]));
    HIP_TRY(h, hipStreamSynchronize(st));
    const uint64_t n = h->pinned[2];
    if (n > w->rs_n_ids) return fail(h, PO_ERR_HIP, "internal: the set of po_walk_prev_copy does not add up");
    *n_out = n;
    const size_t n_give = (size_t)std::min<uint64_t>(cap, n);
    if (!n_give || !ids_out) return PO_OK;
    PO_TRY(ensure(h, w->d_rs_step[RS_PIN], (n + 1) * 4, 1.0, false));
    uint32_t* out = w->d_rs_step[RS_PIN].as<uint32_t>();
    hipLaunchKernelGGL(po::k_rr_list, dim3(stride_grid(h, W)), dim3(256), 0, st, bits, rank, W, out, (uint32_t)n);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(ids_out, out, n_give * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    return PO_OK;
}

// ---- the sequences of graph paths (po_spell): pieces (oriented read, take) -> the bytes of every sequence ------------------

// What po_spell refuses, checked on the host before the device is touched: "" when the input is a valid one.  *n_bytes gets
// the sum of the takes, *n_patched the exception records that lie inside a piece.
std::string spell_check(const po_handle* h, const po_spell_input& in, uint64_t* n_bytes, uint64_t* n_patched) {
    const std::string name = "po_spell: ";
    *n_bytes = *n_patched = 0;
    if (h->segments_only) return name + "the sequences of this handle were added by po_add_segment: they have lengths and no bases";
    if (!in.seq_off || (in.n_pieces && (!in.piece_read || !in.piece_take))) return name + "an input array is missing";
    if (in.seq_off[0] != 0 || in.seq_off[in.n_seqs] != in.n_pieces) return name + "seq_off does not run from 0 to n_pieces";
    for (uint64_t s = 0; s < in.n_seqs; ++s)
        if (in.seq_off[s] > in.seq_off[s + 1]) return name + "seq_off is not ascending at sequence " + std::to_string(s);
    const uint64_t n_reads = h->len.size();
    const bool exc = h->bits == 2 && !h->exc_pos.empty();
    for (uint64_t p = 0; p < in.n_pieces; ++p) {
        const uint32_t r = in.piece_read[p], take = in.piece_take[p];
        if (r >= n_reads) return name + "piece " + std::to_string(p) + " names read " + std::to_string(r) + ", the handle holds " + std::to_string(n_reads);
        if (take > h->len[r])
            return name + "piece " + std::to_string(p) + " takes " + std::to_string(take) + " bytes of a read of " + std::to_string(h->len[r]);
        *n_bytes += take;
        if (exc && h->exc_off[r] != h->exc_off[r + 1]) {
            const uint32_t* e0 = h->exc_pos.data() + h->exc_off[r];
            *n_patched += (uint64_t)(std::lower_bound(e0, h->exc_pos.data() + h->exc_off[r + 1], take) - e0);
        }
    }
    return "";
}

constexpr uint64_t SPELL_MAX_BYTES = 0xFFFFFFFFull - 15;   // 2^32 - 16: the scan of the takes is the library's 32-bit one

po_status run_spell(po_handle* h, const po_spell_input& in, uint64_t n_bytes, uint64_t n_patched, po_result* r) {
    hipStream_t st = h->stream;
    po_spell_stats& S = h->spstats;
    S = po_spell_stats();
    r->special = 3;
    r->elem = 1;
    const uint32_t n_seqs = (uint32_t)in.n_seqs, n = (uint32_t)in.n_pieces;
    if (n) PO_TRY(upload(h));   // (the reads, if they changed since the last upload)
    PO_TRY(lay_events(h));
    hipEvent_t* ev = h->ev_lay + EV_SPELL;
    DevBuf* B = h->d_sp;
    // the input as one upload out of page-locked memory: [seq_off | piece_read | piece_take]
    const size_t soff_bytes = ((size_t)n_seqs + 1) * 8, in_bytes = soff_bytes + (size_t)n * 8;
    const uint64_t n_chunks = (n_bytes + 15) / 16;
    PO_TRY(ensure_host(h, h->scratch_host, std::max(in_bytes, soff_bytes)));
    char* land = static_cast<char*>(h->scratch_host.p);
    std::memcpy(land, in.seq_off, soff_bytes);
    if (n) {
        std::memcpy(land + soff_bytes, in.piece_read, (size_t)n * 4);
        std::memcpy(land + soff_bytes + (size_t)n * 4, in.piece_take, (size_t)n * 4);
    }
    PO_TRY(ensure(h, h->d_scalars, 128));
    PO_TRY(ensure(h, B[SB_IN], in_bytes));
    PO_TRY(ensure(h, B[SB_SCAN], ((size_t)n + 1) * 4));
    PO_TRY(ensure(h, B[SB_POFF], ((size_t)n + 1) * 8));
    PO_TRY(ensure(h, B[SB_SOFF], soff_bytes));
    if (h->spare_spell.p && h->spare_spell.cap >= n_chunks * 16) {
        r->d_rows = h->spare_spell;
        h->spare_spell = DevBuf();
    }
    PO_TRY(ensure(h, r->d_rows, std::max<size_t>(n_chunks * 16, 256), 1.0, false));
    const uint64_t* d_seq_off = B[SB_IN].as<uint64_t>();
    const uint32_t* d_read = reinterpret_cast<const uint32_t*>(B[SB_IN].as<char>() + soff_bytes);
    const uint32_t* d_take = d_read + n;
    uint32_t* scan = B[SB_SCAN].as<uint32_t>();
    uint64_t *poff = B[SB_POFF].as<uint64_t>(), *soff = B[SB_SOFF].as<uint64_t>();
    HIP_TRY(h, hipEventRecord(ev[0], st));
    HIP_TRY(h, hipMemcpyAsync(B[SB_IN].p, land, in_bytes, hipMemcpyHostToDevice, st));
    PO_TRY(prefix_sum<uint32_t>(h, d_take, n, scan, &h->pinned[2]));
    hipLaunchKernelGGL(po::k_spell_offsets, dim3(stride_grid(h, (uint64_t)std::max(n, n_seqs) + 1)), dim3(256), 0, st, n ? scan : nullptr, n, d_seq_off,
                       n_seqs, poff, soff);
    if (n_chunks) {
        const uint64_t* words = h->d_words.as<uint64_t>();
        const uint64_t* woff = h->d_woff.as<uint64_t>();
        po::SpellChunk* out = r->d_rows.as<po::SpellChunk>();
        const dim3 grid(stride_grid(h, n_chunks));
        hipLaunchKernelGGL(po::k_spell_decode, grid, dim3(256), 0, st, words, woff, (uint32_t)h->bits, d_read, d_take, poff, n, 0ull, n_chunks, out);
        if (h->bits == 2 && h->n_exc_uploaded)
            hipLaunchKernelGGL(po::k_spell_patch, dim3(stride_grid(h, n)), dim3(256), 0, st, d_read, d_take, poff, n, h->d_exc_off.as<uint32_t>(),
                               h->d_exc_pos.as<uint32_t>(), h->d_exc_byte.as<uint8_t>(), 0ull, n_chunks * 16, r->d_rows.as<uint8_t>());
    }
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(ev[1], st));
    // (the input has left the landing zone: the stream is in order)
    HIP_TRY(h, hipMemcpyAsync(land, soff, soff_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    r->sp_off.assign(reinterpret_cast<const uint64_t*>(land), reinterpret_cast<const uint64_t*>(land) + n_seqs + 1);
    if ((n && h->pinned[2] != n_bytes) || r->sp_off[0] != 0 || r->sp_off[n_seqs] != n_bytes)
        return fail(h, PO_ERR_HIP, "internal: the offsets of po_spell do not add up");
    S.n_seqs = n_seqs;
    S.n_pieces = n;
    S.n_bytes = n_bytes;
    S.n_patched = n_patched;
    (void)hipEventElapsedTime(&S.device_ms, ev[0], ev[1]);
    return PO_OK;
}

// ---- what the po_layout_* entry points share ------------------------------------------------------------------------

// Everything an edge-producing entry point does behind its checks: `run(result)` fills a new result of handle h, which
// goes to *out; a failed call leaves nothing behind on the device and no result.
template <class Run>
po_status new_edge_result(po_handle* h, const char* name, po_result** out, Run&& run) {
    po_result* r = new (std::nothrow) po_result();
    if (!r) return fail(h, PO_ERR_NOMEM, "out of host memory");
    r->h = h;
    po_status st;
    try {
        st = run(r);
    } catch (const std::bad_alloc&) {
        st = fail(h, PO_ERR_NOMEM, std::string("out of host memory in ") + name);
    }
    if (st != PO_OK) {
        if (h->dev_ready) (void)hipStreamSynchronize(h->stream);
        release_device(r);
        delete r;
        return st;
    }
    ++h->live_results;
    *out = r;
    return PO_OK;
}

// A stage-2 entry point behind its null checks: the checks every stage makes, in the order the messages promise, then
// the call.  `needs` and `merged_msg` end the two sentences that differ from stage to stage.
template <class Run>
po_status stage2_call(po_handle* h, po_result* edges, const char* name, bool params_ok, const char* needs, const char* merged_msg,
                      po_result** out, Run&& run) {
    if (edges->h != h) return fail(h, PO_ERR_INVALID, std::string(name) + ": the edges belong to another handle");
    if (!params_ok) return fail(h, PO_ERR_INVALID, std::string(name) + ": bad parameters");
    // (no CPU fallback: without a usable GPU nothing below can be true of a result either)
    PO_TRY(init_device(h));
    if (edges->elem != sizeof(po_edge) || !edges->kind_edges || edges->host_graph)
        return fail(h, PO_ERR_INVALID, std::string(name) + " needs " + needs);
    if (edges->merged) return fail(h, PO_ERR_INVALID, std::string(name) + ": " + merged_msg);
    return new_edge_result(h, name, out, run);
}

constexpr const char* CANNOT_CLEAN_AGAIN = "a merged graph (po_layout_merge) cannot be cleaned again";

// What an entry point that fills the caller's arrays does behind its checks: the driver under the `bad_alloc` guard; a
// failed call leaves nothing in flight on the stream.
template <class Run>
po_status guarded_run(po_handle* h, const char* name, Run&& run) {
    po_status st;
    try {
        st = run();
    } catch (const std::bad_alloc&) {
        st = fail(h, PO_ERR_NOMEM, std::string("out of host memory in ") + name);
    }
    if (st != PO_OK && h->dev_ready) (void)hipStreamSynchronize(h->stream);
    return st;
}

// An analysis entry point on a graph result (po_layout_components, po_layout_partition): the checks both make, in the
// order the messages promise, then the call.  `counted` ends the sentence about the count the caller must take.
template <class Run>
po_status graph_call(po_handle* h, po_result* graph, const char* name, bool params_ok, const char* counted, uint64_t* count_out,
                     Run&& run) {
    if (!h || !graph) return PO_ERR_INVALID;
    if (!count_out) return fail(h, PO_ERR_INVALID, std::string(name) + ": no room for the number of " + counted);
    *count_out = 0;
    if (graph->h != h) return fail(h, PO_ERR_INVALID, std::string(name) + ": the graph belongs to another handle");
    if (!params_ok) return fail(h, PO_ERR_INVALID, std::string(name) + ": bad parameters");
    if (graph->elem != sizeof(po_edge) || !graph->kind_edges)
        return fail(h, PO_ERR_INVALID, std::string(name) + " needs an edge result, a merged graph or a po_graph_from_edges result");
    // (no CPU fallback)
    PO_TRY(init_device(h));
    return guarded_run(h, name, run);
}

template <class S>
po_status get_stats(const po_handle* h, S po_handle::*member, S* out) {
    if (!h || !out) return PO_ERR_INVALID;
    *out = h->*member;
    return PO_OK;
}

// ---- GFA2 reader for `phasm layout` (S and E lines) ---------------------------------------------

struct Field {
    const char* p;
    size_t n;
};

// Python's line.strip().split('\t'), then .strip() of a field
inline void strip(const char*& p, size_t& n) {
    auto ws = [](char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\f' || c == '\v'; };
    while (n && ws(p[0])) ++p, --n;
    while (n && ws(p[n - 1])) --n;
}

size_t split_tabs(const char* p, size_t n, Field* out, size_t max_fields) {
    strip(p, n);
    size_t k = 0;
    const char* f0 = p;
    for (size_t i = 0; i <= n; ++i) {
        if (i == n || p[i] == '\t') {
            if (k < max_fields) out[k] = Field{f0, (size_t)(p + i - f0)};
            ++k;
            f0 = p + i + 1;
        }
    }
    return k;
}

// int(text) for a decimal field (optional sign, surrounding blanks); _gfa_pos_to_int (gfa.py:65-69) drops one
// trailing '$' first
bool parse_int(Field f, bool allow_dollar, long long& out) {
    const char* p = f.p;
    size_t n = f.n;
    if (allow_dollar && n && p[n - 1] == '$') --n;
    strip(p, n);
    if (!n) return false;
    bool neg = false;
    if (*p == '+' || *p == '-') {
        neg = *p == '-';
        ++p, --n;
    }
    if (!n || n > 18) return false;
    long long v = 0;
    for (size_t i = 0; i < n; ++i) {
        if (p[i] < '0' || p[i] > '9') return false;
        v = v * 10 + (p[i] - '0');
    }
    out = neg ? -v : v;
    return true;
}

// name -> read index (the reference keeps a dict, gfa.py:107-109)
struct NameIndex {
    std::vector<uint32_t> slot;  // read index + 1, 0 = empty
    uint32_t mask = 0;
    static uint64_t hash(const char* p, size_t n) {
        uint64_t x = 1469598103934665603ull;
        for (size_t i = 0; i < n; ++i) x = (x ^ (unsigned char)p[i]) * 1099511628211ull;
        return x ^ (x >> 29);
    }
    void build(const po_handle* h) {
        const size_t n_names = h->ids.size() / 2;
        size_t cap = 16;
        while (cap < 2 * n_names + 2) cap <<= 1;
        slot.assign(cap, 0);
        mask = (uint32_t)(cap - 1);
        for (size_t i = 0; i < n_names; ++i) {
            const std::string& id = h->ids[2 * i];
            uint32_t s = (uint32_t)hash(id.data(), id.size() - 1) & mask;
            while (slot[s]) s = (s + 1) & mask;
            slot[s] = (uint32_t)i + 1;
        }
    }
    long find(const po_handle* h, const char* p, size_t n) const {
        uint32_t s = (uint32_t)hash(p, n) & mask;
        while (slot[s]) {
            const std::string& id = h->ids[2 * (size_t)(slot[s] - 1)];
            if (id.size() - 1 == n && std::memcmp(id.data(), p, n) == 0) return (long)slot[s] - 1;
            s = (s + 1) & mask;
        }
        return -1;
    }
};

po_status add_segment(po_handle* h, const char* name, size_t name_len, uint32_t length) {
    if (!h->len.empty() && !h->segments_only)
        return fail(h, PO_ERR_INVALID, "this handle already holds sequences; segments need a handle of their own");
    if (h->len.size() >= 0xFFFFFFF0ull - 2) return fail(h, PO_ERR_CAPACITY, "too many reads");
    h->segments_only = true;
    std::string id(name ? name : "", name_len);
    id.push_back('+');
    h->ids.push_back(id);
    id.back() = '-';
    h->ids.push_back(id);
    h->len.push_back(length);
    h->len.push_back(length);
    h->total_bases += 2ull * length;
    h->ids_paired = -1;
    return PO_OK;
}


// ---- parallel FASTA ingest (pure-ACGT files, the common case) -------------------------------------
// po_add_fasta's sequential path parses, reverse-complements and packs one record after the other: 0.9 s for the
// 715 MB of config 2, the longest part of the `overlap` command.  Here one pass over the mapped file finds the
// records and their lengths, the packed store is sized once, and a few threads gather / reverse-complement / pack
// the records into their final places.  Any byte outside upper-case ACGT (exception records, pairing checks), an
// 8-bit handle or a handle that already holds exception records makes it step aside for the sequential path:
// returns false with the handle untouched.
struct FastaRec {
    const char* name;
    size_t name_len;
    const char* seq_begin;  // first byte after the header line
    const char* seq_end;    // start of the next header (or end of file)
    size_t seq_len;         // bases once lines are joined and blanks trimmed
};

// what handle_line does to a sequence line: cut \r\n, then blanks at both ends
inline void trim_seq_line(const char*& p, size_t& n) {
    while (n && (p[n - 1] == '\r' || p[n - 1] == '\n')) --n;
    while (n && (p[n - 1] == ' ' || p[n - 1] == '\t')) --n;
    while (n && (p[0] == ' ' || p[0] == '\t')) ++p, --n;
}

bool add_fasta_parallel(po_handle* h, const char* data, size_t size, uint64_t* n_records) {
    if (h->bits != 2 || !h->exc_pos.empty()) return false;
    std::vector<FastaRec> recs;
    {   // pass A: records, in file order.  The file is cut into ranges; a range's thread takes the records whose header
        // line STARTS inside the range and follows its last record to the next header (or the end of the file) -- one
        // thread over the 715 MB of config 2 was 0.15 s of the command's 0.19 s of ingest
        // (threads: the process's CPU share less the two that bring the device up and register the stores beside this)
        const unsigned hw = std::max(1u, cpu_share() > 3 ? cpu_share() - 2 : cpu_share());
        unsigned n_rng = (unsigned)std::max<size_t>(1, std::min<size_t>(std::min(hw, 16u), size >> 22));
        if (const char* e = getenv("PHASM_FASTA_RANGES")) n_rng = (unsigned)std::max(1, std::min(64, atoi(e)));   // (tests: many ranges on small files)
        if ((size_t)n_rng > size) n_rng = 1;
        std::vector<std::vector<FastaRec>> part(n_rng);
        auto scan = [&](unsigned k) {
            const size_t lo = size / n_rng * k, hi = k + 1 == n_rng ? size : size / n_rng * (k + 1);
            size_t pos = lo;
            if (lo) {   // first line start at or after lo
                const char* nl = static_cast<const char*>(std::memchr(data + lo - 1, '\n', size - (lo - 1)));
                pos = nl ? (size_t)(nl - data) + 1 : size;
            }
            std::vector<FastaRec>& out = part[k];
            bool have = false;
            while (pos < size) {
                const char* nl = static_cast<const char*>(std::memchr(data + pos, '\n', size - pos));
                const size_t len = nl ? (size_t)(nl - (data + pos)) + 1 : size - pos;
                const char* p = data + pos;
                size_t n = len;
                while (n && (p[n - 1] == '\r' || p[n - 1] == '\n')) --n;
                if (n && p[0] == '>') {
                    if (have) out.back().seq_end = data + pos;
                    if (pos >= hi) return;   // the next range's first record
                    out.push_back(FastaRec{p + 1, n - 1, data + pos + len, data + size, 0});
                    have = true;
                } else if (n && have) {
                    size_t m = len;
                    trim_seq_line(p, m);
                    out.back().seq_len += m;
                } else if (!have && pos >= hi) {
                    return;                  // (no header started in this range)
                }
                pos += len;
            }
        };
        std::vector<std::thread> thr;
        try {
            for (unsigned k = 1; k < n_rng; ++k) thr.emplace_back(scan, k);
        } catch (const std::system_error&) {
        }
        const unsigned started = (unsigned)thr.size() + 1;
        scan(0);
        for (auto& th : thr) th.join();
        for (unsigned k = started; k < n_rng; ++k) scan(k);   // (threads that could not be started)
        size_t total = 0;
        for (const auto& v : part) total += v.size();
        recs.reserve(total);
        for (auto& v : part) recs.insert(recs.end(), v.begin(), v.end());
    }
    if (getenv("PHASM_FASTA_TRACE")) std::fprintf(stderr, "[fasta] %zu records found\n", recs.size());
    if (recs.empty()) {
        if (n_records) *n_records = 0;
        return true;
    }
    for (const FastaRec& r : recs)
        if (r.seq_len > 0x7FFFFFF0ull) return false;  // (the sequential path reports it)
    if (h->len.size() + 2 * recs.size() >= 0xFFFFFFF0ull) return false;
    // final place of every oriented read in its packed store (append_packed's layout): forward reads go to the
    // store of the next read's parity, reverse complements to the other one
    if (h->len.size() & 1) return false;  // (an odd number of reads so far: pairs would straddle the stores; sequential path)
    const size_t old_words[2] = {h->words[0].size(), h->words[1].size()};
    std::vector<size_t> off(2 * recs.size());
    size_t cur[2] = {old_words[0], old_words[1]};
    for (size_t i = 0; i < recs.size(); ++i) {
        const size_t nw = (recs[i].seq_len + 31) / 32;
        for (int k = 0; k < 2; ++k) {
            const size_t o = (cur[k] + 1) & ~size_t(1);
            off[2 * i + k] = o;
            cur[k] = o + nw + 1;
        }
    }
    const bool ftrace = getenv("PHASM_FASTA_TRACE") != nullptr;
    const auto ft0 = std::chrono::steady_clock::now();
    auto fmark = [&](const char* what) {
        if (ftrace) std::fprintf(stderr, "[fasta] %s at %.1f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ft0).count());
    };
    // the stores grow WITHOUT being zero-filled and without being page-locked here: the packing threads below write every
    // word (first touch in parallel), and the registration runs beside them on a thread of its own (RegAlloc::reg_now)
    g_reg_defer = true;
    try {
        h->words[0].resize(cur[0]);
        h->words[1].resize(cur[1]);
    } catch (...) {
        g_reg_defer = false;
        throw;
    }
    g_reg_defer = false;
    fmark("stores sized");
    uint64_t* words[2] = {h->words[0].data(), h->words[1].data()};
    std::thread reg_thread;
    try {
        uint64_t* blocks[2] = {h->words[0].capacity() ? words[0] : nullptr, h->words[1].capacity() ? words[1] : nullptr};
        reg_thread = std::thread([blocks, &fmark] {
            for (int k = 0; k < 2; ++k)
                if (blocks[k]) RegAlloc<uint64_t>::reg_now(blocks[k]);
            fmark("stores registered");
        });
    } catch (const std::system_error&) {
    }
    struct RegJoin {
        std::thread& t;
        po_handle* h;
        ~RegJoin() {
            if (t.joinable()) t.join();
            else   // (no thread: register here)
                for (int k = 0; k < 2; ++k)
                    if (h->words[k].capacity()) RegAlloc<uint64_t>::reg_now(h->words[k].data());
        }
    } reg_join{reg_thread, h};
    const uint8_t* lut = g_lut.v;
    const unsigned char* comp = comp_table();
    std::atomic<size_t> next{0};
    std::atomic<int> bad{0};
    auto pack = [&](const unsigned char* sq, size_t n, uint64_t* w) -> uint8_t {
        uint8_t b = 0;
        const size_t full = n / 32;
        for (size_t k = 0; k < full; ++k) {
            const unsigned char* q = sq + k * 32;
            uint64_t acc = 0;
            for (int j = 0; j < 32; ++j) {
                const uint8_t c = lut[q[j]];
                b |= c;
                acc |= (uint64_t)(c & 3) << (2 * j);
            }
            w[k] = acc;
        }
        if (full * 32 < n) {
            uint64_t acc = 0;
            for (size_t i = full * 32; i < n; ++i) {
                const uint8_t c = lut[sq[i]];
                b |= c;
                acc |= (uint64_t)(c & 3) << (2 * (i & 31));
            }
            w[full] = acc;
        }
        return b;
    };
    auto worker = [&]() {
      try {
        std::string seq, rc;
        for (;;) {
            const size_t lo = next.fetch_add(64);
            if (lo >= recs.size() || bad.load(std::memory_order_relaxed)) return;
            const size_t hi = std::min(recs.size(), lo + 64);
            for (size_t i = lo; i < hi; ++i) {
                const FastaRec& r = recs[i];
                seq.clear();
                seq.reserve(r.seq_len);
                for (const char* p = r.seq_begin; p < r.seq_end;) {
                    const char* nl = static_cast<const char*>(std::memchr(p, '\n', (size_t)(r.seq_end - p)));
                    size_t n = nl ? (size_t)(nl - p) + 1 : (size_t)(r.seq_end - p);
                    const char* q = p;
                    size_t m = n;
                    trim_seq_line(q, m);
                    seq.append(q, m);
                    p += n;
                }
                const size_t n = seq.size();
                if (n != r.seq_len) {  // (pass A sized the stores with seq_len: never pack anything else into them)
                    bad.store(1);
                    return;
                }
                rc.resize(n);
                for (size_t k = 0; k < n; ++k) rc[k] = (char)comp[(unsigned char)seq[n - 1 - k]];
                // (the words between the reads: the alignment gap in front, if there is one, and the spare word behind)
                const size_t nw = (n + 31) / 32;
                for (int k = 0; k < 2; ++k) {
                    const size_t prev_end = i ? off[2 * (i - 1) + k] + (recs[i - 1].seq_len + 31) / 32 + 1 : old_words[k];
                    if (off[2 * i + k] > prev_end) words[k][off[2 * i + k] - 1] = 0;
                    words[k][off[2 * i + k] + nw] = 0;
                }
                uint8_t b = pack(reinterpret_cast<const unsigned char*>(seq.data()), n, words[0] + off[2 * i]);
                b |= pack(reinterpret_cast<const unsigned char*>(rc.data()), n, words[1] + off[2 * i + 1]);
                if (n != r.seq_len || (b & 0x80)) {
                    bad.store(1);
                    return;
                }
            }
        }
      } catch (...) {
        bad.store(1);  // (out of memory in a worker: the sequential path will report it)
      }
    };
    {
        const unsigned hw = std::max(1u, cpu_share() > 3 ? cpu_share() - 2 : cpu_share());
        const unsigned n_thr = std::max(1u, std::min(hw, 16u));
        std::vector<std::thread> thr;
        try {
            for (unsigned t = 1; t < n_thr; ++t) thr.emplace_back(worker);
        } catch (const std::system_error&) {
            // fewer threads than asked for: carry on with those that started
        }
        worker();
        for (auto& th : thr) th.join();
    }
    fmark("packed");
    if (bad.load()) {  // something other than upper-case ACGT: let the sequential path deal with it
        h->words[0].resize(old_words[0]);
        h->words[1].resize(old_words[1]);
        return false;
    }
    h->ids.reserve(h->ids.size() + 2 * recs.size());
    for (size_t i = 0; i < recs.size(); ++i) {
        std::string id(recs[i].name, recs[i].name_len);
        id.push_back('+');
        h->ids.push_back(id);
        id.back() = '-';
        h->ids.push_back(std::move(id));
        for (int k = 0; k < 2; ++k) {
            h->len.push_back((uint32_t)recs[i].seq_len);
            h->woff.push_back(off[2 * i + k]);
            h->exc_off.push_back((uint32_t)h->exc_pos.size());
        }
        h->total_bases += 2 * recs[i].seq_len;
    }
    h->dirty = true;
    h->ids_paired = -1;
    if (n_records) *n_records = recs.size();
    fmark("ids and tables appended");
    return true;
}

}  // namespace

extern "C" {

int po_abi_version(void) { return PO_ABI_VERSION; }

po_status po_create(po_handle** out) {
    if (!out) return PO_ERR_INVALID;
    po_handle* h = new (std::nothrow) po_handle();
    if (!h) return PO_ERR_NOMEM;
    *out = h;
    return PO_OK;
}

void po_destroy(po_handle* h) {
    if (!h) return;
    if (h->dev_ready) {
        (void)hipSetDevice(h->device);
        (void)hipStreamSynchronize(h->stream);
        DevBuf* bufs[] = {&h->d_words, &h->d_woff, &h->d_len, &h->d_tiles, &h->d_read_tile0, &h->d_left, &h->d_left_cnt, &h->d_tile_extra, &h->d_exc_off, &h->d_exc_pos, &h->d_exc_byte, &h->d_pair_state, &h->d_truemask,
                          &h->d_table, &h->d_slot_cnt, &h->d_slot_cur, &h->d_slot_start, &h->d_read_slot, &h->d_chain,
                          &h->d_chain_tmp, &h->d_long_list, &h->d_entry_off, &h->d_bloom, &h->d_selfrep, &h->d_tile_count, &h->d_tile_off,
                          &h->d_ps_blocks, &h->d_scalars, &h->d_cand_a, &h->d_cand_p, &h->d_cand_b, &h->d_type,
                          &h->d_rowcnt, &h->d_row_off, &h->d_flag, &h->d_pair_key, &h->d_pair_min, &h->spare_rows, &h->spare_cands, &h->spare_edges, &h->spare_nrank, &h->spare_spell,
                          &h->d_vlabel, &h->d_vrank, &h->d_vperm, &h->d_end_a, &h->d_end_b, &h->d_dpcnt, &h->d_lay_len, &h->d_lay_cnt, &h->d_rflag, &h->d_removed, &h->d_ekey, &h->d_ecnt,
                          &h->d_ewin, &h->d_eoff, &h->d_chain_state, &h->d_tail_state, &h->d_efirst, &h->d_lay_firstc};
        // every stream idle before anything the device (or a copy) may still touch is given back
        if (h->copy_stream) (void)hipStreamSynchronize(h->copy_stream);
        if (h->up_stream) (void)hipStreamSynchronize(h->up_stream);
        if (h->rc_stream) (void)hipStreamSynchronize(h->rc_stream);
        for (DevBuf* b : bufs) b->release();
        for (DevBuf& b : h->d_red) b.release();
        for (DevBuf& b : h->d_tip) b.release();
        for (DevBuf& b : h->d_mrg) b.release();
        for (DevBuf& b : h->d_cov) b.release();
        for (DevBuf& b : h->d_rank) b.release();
        for (DevBuf& b : h->d_cc) b.release();
        for (DevBuf& b : h->d_scc) b.release();
        for (DevBuf& b : h->d_sb) b.release();
        for (DevBuf& b : h->d_cy) b.release();
        for (DevBuf& b : h->d_bc) b.release();
        for (DevBuf& b : h->d_ct) b.release();
        for (DevBuf& b : h->d_ph) b.release();
        for (DevBuf& b : h->d_rr) b.release();
        for (DevBuf& b : h->d_sp) b.release();
        for (DevBuf& b : h->d_pp) b.release();
        for (DevBuf& b : h->d_lg) b.release();
        const bool pooled = kit_give(h);
        if (!pooled) {
        for (int i = 0; i < 2 * EV_N; ++i) (void)hipEventDestroy(h->ev_sets[i / EV_N][i % EV_N]);
        for (hipEvent_t e : h->ev_lay)
            if (e) (void)hipEventDestroy(e);
        (void)hipEventDestroy(h->ev_up0);
        (void)hipEventDestroy(h->ev_up1);
        if (h->pinned) {
            pin_drop(h->pinned);
            (void)hipHostFree(h->pinned);
        }
        }
        h->spare_host.release();
        h->scratch_host.release();
        h->home_stage.release();
        for (DevBuf& b : h->chunk_rows) b.release();
        h->d_first.release();
        h->d_defer.release();
        h->meta_host.release();
        h->stage_host.release();
        for (void* c : h->arena_chunks) (void)hipFree(c);
        h->arena_chunks.clear();
        if (!pooled) {
        if (h->up_stream) {
            (void)hipStreamSynchronize(h->up_stream);
            (void)hipStreamDestroy(h->up_stream);
        }
        for (hipEvent_t e : h->ev_piece)
            if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : h->ev_rc)
            if (e) (void)hipEventDestroy(e);
        if (h->ev_meta) (void)hipEventDestroy(h->ev_meta);
        if (h->rc_stream) {
            (void)hipStreamSynchronize(h->rc_stream);
            (void)hipStreamDestroy(h->rc_stream);
        }
        if (h->ev_first) (void)hipEventDestroy(h->ev_first);
        if (h->copy_stream) {
            (void)hipStreamSynchronize(h->copy_stream);
            (void)hipStreamDestroy(h->copy_stream);
        }
        (void)hipStreamDestroy(h->stream);
        }
    }
    h->spare_host.release();   // (the result pool may exist without the handle ever having made a call)
    h->home_stage.release();
    delete h;
}

po_status po_set_device(po_handle* h, int device) {
    if (!h) return PO_ERR_INVALID;
    if (h->dev_ready && device != h->device) return fail(h, PO_ERR_INVALID, "device already initialised");
    h->device = device;
    return PO_OK;
}

po_status po_add_sequence(po_handle* h, const char* id, size_t id_len, const char* seq, size_t seq_len) {
    if (!h || (!id && id_len) || (!seq && seq_len)) return PO_ERR_INVALID;
    if (h->segments_only) return fail(h, PO_ERR_INVALID, "this handle holds GFA segments (no sequences); use a new handle");
    if (seq_len > 0x7FFFFFF0ull) return fail(h, PO_ERR_CAPACITY, "read longer than 2^31 bases");
    if (h->len.size() >= 0xFFFFFFF0ull) return fail(h, PO_ERR_CAPACITY, "too many reads");
    quiesce_store(h);  // (the store may move)
    try {
        const unsigned char* s = reinterpret_cast<const unsigned char*>(seq);
        if (h->bits != 2 || !append_packed(h, s, seq_len, 2)) {
            if (h->bits == 2) widen_to_bytes(h);  // first non-ACGT byte: everything moves to 8 bits/base
            append_packed(h, s, seq_len, 8);
        }
        h->ids.emplace_back(id ? id : "", id_len);
        h->len.push_back((uint32_t)seq_len);
        h->total_bases += seq_len;
        h->dirty = true;
        h->ids_paired = -1;
        if (h->total_bases >= h->pool_bases && h->total_bases >= (64ull << 20)) result_pool_grow(h);
        if (h->bits == 2 && h->first_n + 1 == h->len.size()) note_first_words(h);   // (O(1): this read's two words)
        if (h->bits == 2 && (h->len.size() & 1) == 0) {
            const size_t r = h->len.size() - 1;
            if (!h->exc_pos.empty()) host_pair_check(h, r, s);
            const bool has_exc = h->exc_off[r - 1] != h->exc_off[r] || h->exc_off[r] != h->exc_off[r + 1];
            if (h->all_pairs_rcx) {
                const bool ok = has_exc ? (h->pair_state.size() > r / 2 && h->pair_state[r / 2] == 1) : packed_is_revcomp(h, r);
                h->all_pairs_rcx = ok;
                if (has_exc || !ok) h->all_pairs_rc = false;
            } else {
                h->all_pairs_rc = false;
            }
        }
    } catch (const std::bad_alloc&) {
        return fail(h, PO_ERR_NOMEM, "out of host memory in po_add_sequence");
    }
    return PO_OK;
}

// FASTA ingest for the overlap command (the reference delegates this to dinopy.FastaReader and
// dinopy.reverse_complement, assembler.py:32-40): header = the whole line after '>', sequence lines
// concatenated, blank lines skipped, bytes kept as they are; with both_strands every record is added
// as name+"+" / sequence and name+"-" / reverse complement (IUPAC-aware, case preserving).
po_status po_add_fasta(po_handle* h, const char* path, int both_strands, uint64_t* n_records) {
    if (!h || !path) return PO_ERR_INVALID;
    if (n_records) *n_records = 0;
    quiesce_store(h);  // (the store may move)
    if (both_strands && !h->segments_only && !getenv("PHASM_FASTA_SEQUENTIAL")) {
        // fast path: map the file, pack with a few threads (pure upper-case ACGT only; see add_fasta_parallel)
        const int fd = ::open(path, O_RDONLY);
        if (fd < 0) return fail(h, PO_ERR_INVALID, std::string("cannot open ") + path);
        struct stat sb;
        bool done = false;
        if (::fstat(fd, &sb) == 0 && sb.st_size > 0) {
            void* m = ::mmap(nullptr, (size_t)sb.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
            if (m != MAP_FAILED) {
                // A file this size is headed for the GPU: the device comes up (runtime start, streams, events, the first code
                // object: ~0.15 s in a fresh process) and the page-locked result pool is made WHILE the file is parsed and
                // packed, not after it -- the `overlap` command is one process and one call (assembler.py:42).  The pool is
                // sized from the file's size (both strands: at most two oriented bases per byte).
                std::thread warm;
                if ((uint64_t)sb.st_size >= (32ull << 20) && !h->dev_ready && !getenv("PHASM_NO_POOL") && !getenv("PHASM_NO_WARM")) {
                    const uint64_t est_bases = 2ull * (uint64_t)sb.st_size;
                    try {
                        warm = std::thread([h, est_bases] {
                            if (h->total_bases + est_bases >= h->pool_bases) result_pool_grow(h, h->total_bases + est_bases);
                        });
                    } catch (const std::system_error&) {
                    }
                }
                struct Joiner {
                    std::thread& t;
                    ~Joiner() {
                        if (t.joinable()) t.join();
                    }
                } joiner{warm};
                try {
                    const auto tf0 = std::chrono::steady_clock::now();
                    done = add_fasta_parallel(h, static_cast<const char*>(m), (size_t)sb.st_size, n_records);
                    if (getenv("PHASM_FASTA_TRACE")) {
                        const double t_parse = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tf0).count();
                        if (warm.joinable()) warm.join();
                        std::fprintf(stderr, "[fasta] parsed and packed in %.1f ms; the device and the result pool were ready %.1f ms after the start\n", t_parse,
                                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tf0).count());
                    }
                } catch (const std::bad_alloc&) {
                    ::munmap(m, (size_t)sb.st_size);
                    ::close(fd);
                    return fail(h, PO_ERR_NOMEM, "out of host memory in po_add_fasta");
                } catch (const std::system_error&) {
                    done = false;
                }
                ::munmap(m, (size_t)sb.st_size);
            }
        }
        ::close(fd);
        if (done) {
            if (h->total_bases >= h->pool_bases && h->total_bases >= (64ull << 20)) result_pool_grow(h);
            if (h->bits == 2) note_first_words(h);
            return PO_OK;
        }
    }
    FILE* f = std::fopen(path, "rb");
    if (!f) return fail(h, PO_ERR_INVALID, std::string("cannot open ") + path);
    const unsigned char* comp = comp_table();
    po_status st = PO_OK;
    uint64_t nrec = 0;
    try {
        std::string name, seq, rc, line;
        bool have = false;
        std::vector<char> buf(1 << 22);
        auto flush_record = [&]() -> po_status {
            if (!have) return PO_OK;
            ++nrec;
            if (!both_strands) return po_add_sequence(h, name.data(), name.size(), seq.data(), seq.size());
            std::string id = name + "+";
            po_status s1 = po_add_sequence(h, id.data(), id.size(), seq.data(), seq.size());
            if (s1 != PO_OK) return s1;
            rc.resize(seq.size());
            for (size_t i = 0, n = seq.size(); i < n; ++i) rc[i] = (char)comp[(unsigned char)seq[n - 1 - i]];
            id.back() = '-';
            return po_add_sequence(h, id.data(), id.size(), rc.data(), rc.size());
        };
        auto handle_line = [&](const char* p, size_t n) -> po_status {
            while (n && (p[n - 1] == '\r' || p[n - 1] == '\n')) --n;
            if (n == 0) return PO_OK;
            if (p[0] == '>') {
                po_status s1 = flush_record();
                if (s1 != PO_OK) return s1;
                name.assign(p + 1, n - 1);
                seq.clear();
                have = true;
            } else if (have) {
                while (n && (p[n - 1] == ' ' || p[n - 1] == '\t')) --n;
                size_t b = 0;
                while (b < n && (p[b] == ' ' || p[b] == '\t')) ++b;
                seq.append(p + b, n - b);
            }
            return PO_OK;
        };
        size_t got;
        while (st == PO_OK && (got = std::fread(buf.data(), 1, buf.size(), f)) > 0) {
            size_t pos = 0;
            while (pos < got && st == PO_OK) {
                const char* nl = static_cast<const char*>(std::memchr(buf.data() + pos, '\n', got - pos));
                if (!nl) {
                    line.append(buf.data() + pos, got - pos);
                    pos = got;
                } else {
                    const size_t len = (size_t)(nl - (buf.data() + pos)) + 1;
                    if (line.empty()) {
                        st = handle_line(buf.data() + pos, len);
                    } else {
                        line.append(buf.data() + pos, len);
                        st = handle_line(line.data(), line.size());
                        line.clear();
                    }
                    pos += len;
                }
            }
        }
        if (st == PO_OK && !line.empty()) st = handle_line(line.data(), line.size());
        if (st == PO_OK) st = flush_record();
    } catch (const std::bad_alloc&) {
        st = fail(h, PO_ERR_NOMEM, "out of host memory in po_add_fasta");
    }
    std::fclose(f);
    if (n_records) *n_records = nrec;
    return st;
}

uint32_t po_num_sequences(const po_handle* h) { return h ? (uint32_t)h->len.size() : 0; }

po_status po_get_id(const po_handle* h, uint32_t idx, const char** id, size_t* id_len) {
    if (!h || idx >= h->ids.size() || !id || !id_len) return PO_ERR_INVALID;
    *id = h->ids[idx].data();
    *id_len = h->ids[idx].size();
    return PO_OK;
}

uint32_t po_get_length(const po_handle* h, uint32_t idx) { return (h && idx < h->len.size()) ? h->len[idx] : 0; }

po_status po_upload(po_handle* h) {
    if (!h) return PO_ERR_INVALID;
    po_status st;
    try {
        st = upload(h);
    } catch (const std::bad_alloc&) {
        st = fail(h, PO_ERR_NOMEM, "out of host memory in po_upload");
    }
    // (a failed upload may have copies from the host store in flight: nothing returns before they are done)
    if (st != PO_OK && h->dev_ready) (void)hipStreamSynchronize(h->stream);
    return st;
}

// ---- sharded upload (multi-GPU): each rank brings 1/N of the packed reads over ITS PCIe link, xGMI does the rest ----
po_status po_upload_piece_part(po_handle* h, uint32_t shard, uint32_t nshards, uint32_t part, uint32_t nparts, void* dst_device,
                               uint64_t capacity_words, uint64_t* word_count, int* ok) {
    if (!h || !word_count || !ok || nshards == 0 || shard >= nshards || nparts == 0 || part >= nparts || nparts > 64) return PO_ERR_INVALID;
    *ok = 0;
    *word_count = 0;
    const uint32_t n = (uint32_t)h->len.size();
    // only when store 1 can be rebuilt on the device (every odd read the reverse complement of its even partner)
    if (!(h->bits == 2 && n >= 2 && (n % 2) == 0 && h->all_pairs_rc && h->exc_pos.empty()) || h->segments_only) return PO_OK;
    PO_TRY(init_device(h));
    uint64_t wb = 0, wc = 0;
    try {
        store0_part_range(h, shard, nshards, part, nparts, &wb, &wc);
    } catch (const std::bad_alloc&) {
        return fail(h, PO_ERR_NOMEM, "out of host memory");
    }
    *word_count = wc;
    *ok = 1;
    if (!dst_device) return PO_OK;   // (a query: how many words is this part of the shard's piece?)
    if (wc > capacity_words) return fail(h, PO_ERR_INVALID, "po_upload_piece: the piece does not fit the destination");
    if (wc) {
        // (a store below the registration size is ordinary heap memory: it goes through the page-locked staging block like
        // every other small source -- handed a pageable pointer the runtime would pin the heap range around it)
        const void* src = h->words[0].data() + wb;
        if (!store_is_pinned(h->words[0]) && wc * 8 <= STAGE_MAX) {
            h->stage_used = 0;   // (no copy is in flight: every path that queued one has synchronised)
            PO_TRY(ensure_host(h, h->stage_host, wc * 8 + 64));
            src = staged(h, src, wc * 8);
        }
        HIP_TRY(h, hipMemcpyAsync(dst_device, src, wc * 8, hipMemcpyHostToDevice, h->stream));
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->upload_bytes = (part == 0 ? 0 : h->upload_bytes) + wc * 8;
    return PO_OK;
}

po_status po_upload_piece(po_handle* h, uint32_t shard, uint32_t nshards, void* dst_device, uint64_t capacity_words,
                          uint64_t* word_count, int* ok) {
    return po_upload_piece_part(h, shard, nshards, 0, 1, dst_device, capacity_words, word_count, ok);
}

po_status po_upload_assemble_parts(po_handle* h, const void* pieces_device, uint64_t slot_words, uint32_t nshards, uint32_t nparts) {
    if (!h || !pieces_device || nshards == 0 || nparts == 0 || nparts > 64) return PO_ERR_INVALID;
    h->asm_pieces = static_cast<const uint64_t*>(pieces_device);
    h->asm_slot_words = slot_words;
    h->asm_n = nshards;
    h->asm_parts = nparts;
    h->dirty = true;
    const uint64_t piece_bytes = h->upload_bytes;
    po_status st;
    try {
        st = upload(h);
    } catch (const std::bad_alloc&) {
        st = fail(h, PO_ERR_NOMEM, "out of host memory in po_upload_assemble");
    }
    h->asm_pieces = nullptr;
    h->asm_parts = 1;
    if (st != PO_OK && h->dev_ready) (void)hipStreamSynchronize(h->stream);
    if (st == PO_OK) {
        h->upload_bytes += piece_bytes;   // (what THIS rank moved over PCIe: its piece + the per-read tables)
        h->stats.upload_bytes = h->upload_bytes;
    }
    return st;
}

po_status po_upload_assemble(po_handle* h, const void* pieces_device, uint64_t slot_words, uint32_t nshards) {
    return po_upload_assemble_parts(h, pieces_device, slot_words, nshards, 1);
}

po_status po_invalidate(po_handle* h) {
    if (!h) return PO_ERR_INVALID;
    h->dirty = true;
    return PO_OK;
}

static po_status overlaps_common(po_handle* h, const OverlapArgs& a, po_result** out, void* ext_dst = nullptr, uint64_t ext_cap = 0) {
    if (!h || !out) return PO_ERR_INVALID;
    *out = nullptr;
    if (a.nshards == 0 || a.shard >= a.nshards) return fail(h, PO_ERR_INVALID, "shard must be < nshards");
    if (h->segments_only) return fail(h, PO_ERR_INVALID, "this handle holds GFA segments without sequences: nothing to overlap");
    po_result* r = new (std::nothrow) po_result();
    if (!r) return fail(h, PO_ERR_NOMEM, "out of host memory");
    r->h = h;
    r->ext_dst = ext_dst;
    r->ext_cap = ext_cap;
    po_status st;
    try {
        st = upload(h);
        if (st == PO_OK) st = h->bits == 2 ? run_overlaps<2>(h, a, r) : run_overlaps<8>(h, a, r);
    } catch (const std::bad_alloc&) {
        st = fail(h, PO_ERR_NOMEM, "out of host memory in po_overlaps");
    }
    if (st != PO_OK) {
        if (h->dev_ready) (void)hipStreamSynchronize(h->stream);
        r->d_rows.release();
        delete r;
        return st;
    }
    ++h->live_results;
    *out = r;
    return PO_OK;
}

po_status po_overlaps_shard(po_handle* h, uint32_t min_length, uint32_t shard, uint32_t nshards, po_result** out) {
    return overlaps_common(h, OverlapArgs{min_length, shard, nshards, false}, out);
}

po_status po_candidates_shard(po_handle* h, uint32_t min_length, uint32_t shard, uint32_t nshards, po_result** out) {
    return overlaps_common(h, OverlapArgs{min_length, shard, nshards, true}, out);
}

po_status po_candidates_shard_into(po_handle* h, uint32_t min_length, uint32_t shard, uint32_t nshards, void* dst_device,
                                   uint64_t capacity, int* written, po_result** out) {
    if (written) *written = 0;
    if (!dst_device && capacity) return PO_ERR_INVALID;
    const po_status st = overlaps_common(h, OverlapArgs{min_length, shard, nshards, true}, out, dst_device, capacity);
    if (st == PO_OK && written) *written = (*out)->wrote_ext ? 1 : 0;
    return st;
}

po_status po_expand(po_handle* h, const void* candidates_device, uint64_t n_candidates, po_result** out) {
    if (!h || !out || (!candidates_device && n_candidates)) return PO_ERR_INVALID;
    *out = nullptr;
    if (h->segments_only) return fail(h, PO_ERR_INVALID, "this handle holds GFA segments without sequences");
    po_result* r = new (std::nothrow) po_result();
    if (!r) return fail(h, PO_ERR_NOMEM, "out of host memory");
    r->h = h;
    po_status st;
    try {
        st = upload(h);
        if (st == PO_OK) st = run_expand(h, candidates_device, n_candidates, r);
    } catch (const std::bad_alloc&) {
        st = fail(h, PO_ERR_NOMEM, "out of host memory in po_expand");
    }
    if (st != PO_OK) {
        if (h->dev_ready) (void)hipStreamSynchronize(h->stream);
        r->d_rows.release();
        delete r;
        return st;
    }
    ++h->live_results;
    *out = r;
    return PO_OK;
}

po_status po_overlaps(po_handle* h, uint32_t min_length, po_result** out) {
    return po_overlaps_shard(h, min_length, 0, 1, out);
}

// po_overlaps + po_result_rows in one call, pipelined.  Two forms:
//
// * the reads are on the device already: the a-side reads are cut into chunks (the shards of po_overlaps_shard), and
//   while chunk k + 1 goes through the kernels on the handle's stream, chunk k's rows travel device -> host on a
//   second stream into ONE page-locked array;
// * the read set changed since the last upload (what the reference's overlaps() faces every time: the reads are host
//   memory, overlapper.cpp:22-36): the STREAMED step.  The packed reads cross PCIe in pieces, in index order, on a
//   third stream; as soon as piece k is there, its reads are scanned against the whole index (built from every read's
//   first word, which travels ahead: 8 bytes per read), and the pairs whose b-side read has arrived are verified
//   and emitted -- the reversed index order of kernels.hip.h (mirror_rank, mode 3) picks the member of every
//   strand-mirror pair whose b lies at or below its a, so every suffix-prefix candidate of piece k is of that kind --
//   and piece k's rows travel back while piece k + 1 is still coming in: PCIe carries both directions at once.
//   Containments of a read that has not arrived are the only candidates that must wait (the deferred list).
//
// Same rows as po_overlaps as a multiset (which member of a strand-mirror pair is computed differs, the emitted
// pair of rows does not), a-major chunk by chunk.  The result holds the host array only.
extern "C++" {
namespace {

struct HostRows {
    HostBuf hb;
    uint64_t total = 0;
};

// ---- the helper threads of a po_overlaps_to_host call (namespace home) ----
bool home_begin(po_handle* h) {
    h->home_on = false;
    if (!home_enabled()) return false;
    home::Pool* P = home::pool();
    if (!P) return false;
    P->call_mu.lock();
    home::begin(P, h->len.data(), (uint32_t)h->len.size(), getenv("PHASM_STREAM_TRACE") != nullptr || getenv("PHASM_HOME_TRACE") != nullptr);
    h->home_on = true;
    h->home_used = 0;
    h->home_seq = 0;
    // a and b in ceil(log2(reads)) bits each, p in ceil(log2(longest read + 1)), type in the top two: one 64-bit word when
    // that fits (100 k reads of 15 kb: 17 + 17 + 14; 2 M reads of 12 kb: 21 + 21 + 14), the 16-byte record otherwise
    if (h->home_pack_n != h->len.size() || h->home_pack_bases != h->total_bases) {
        uint32_t longest = 0;
        for (uint32_t l : h->len) longest = std::max(longest, l);
        uint32_t br = 1, bp = 1;
        while ((1ull << br) < (uint64_t)h->len.size()) ++br;
        while ((1ull << bp) < (uint64_t)longest + 1ull) ++bp;
        const bool fits = 2 * br + bp <= 62;
        h->home_pack_b = fits ? br : 0u;
        h->home_pack_p = fits ? 2 * br : 0u;
        h->home_pack_n = h->len.size();
        h->home_pack_bases = h->total_bases;
    }
    const char* pk = getenv("PHASM_HOME_PACK");
    const bool pack = !(pk && atoi(pk) == 0);
    h->home_sh_b = pack ? h->home_pack_b : 0u;
    h->home_sh_p = pack ? h->home_pack_p : 0u;
    return true;
}

// every piece submitted so far has been expanded (or the pool has stopped on an error)
void home_wait(po_handle* h) {
    if (h->home_on) home::wait_all(home::g_pool);
}

// returns the pool's error code (0 = fine)
int home_end(po_handle* h, po_stats* sum = nullptr) {
    if (!h->home_on) return 0;
    home::Pool* P = home::g_pool;
    home::wait_all(P);
    const int err = P->error.load();
    if (sum) {   // (the byte counters of the pieces that went home as records)
        sum->sum_overlap_bases += P->sum_l.load();
        sum->verify_bytes_algo += P->sum_b.load();
        sum->verify_bytes_exec += P->sum_e.load();
    }
    if (P->tracing)
        for (size_t i = 0; i < P->trace.size(); ++i)
            std::fprintf(stderr, "[home] piece %zu: records home at %.3f ms, %.0f rows written at %.3f ms (since the call set the pool up)\n", i,
                         P->trace[i][0] * 1e-3, P->trace[i][2], P->trace[i][1] * 1e-3);
    h->home_on = false;
    P->call_mu.unlock();
    return err;
}

// room for `nk` more rows in the page-locked array (first call, or more rows than last time: guess the whole from what has
// been seen, move what is there).  seen_share (streamed step): the share of all (a, b) index pairs the pieces so far
// cover -- rows grow with the SQUARE of the reads that have arrived, a linear guess from the first piece is 6 x short
po_status rows_room(po_handle* h, HostRows& R, uint64_t nk, uint32_t k, uint32_t n_chunks, double seen_share) {
    const size_t need = (size_t)(R.total + nk) * sizeof(po_row);
    if (need <= R.hb.cap) return PO_OK;
    uint64_t guess = std::max<uint64_t>(h->last_host_rows, (R.total + nk) * n_chunks / (k + 1));
    if (seen_share > 0.0) guess = std::max<uint64_t>(guess, (uint64_t)((double)(R.total + nk) / seen_share * 1.05));
    HostBuf bigger;
    PO_TRY(ensure_host(h, bigger, std::max<size_t>(need, (size_t)(guess + guess / 8) * sizeof(po_row))));
    home_wait(h);   // (helper threads may be writing rows into the old array)
    if (hipStreamSynchronize(h->copy_stream) != hipSuccess) {
        bigger.release();
        return fail(h, PO_ERR_HIP, "copy stream");
    }
    if (R.total) std::memcpy(bigger.p, R.hb.p, (size_t)R.total * sizeof(po_row));
    R.hb.release();
    R.hb = bigger;
    return PO_OK;
}

// the rows of one chunk as RECORDS: their copy on the copy stream into the staging block, an event behind it, and the piece
// goes to the helper threads, which write its nk rows at R.total
po_status append_home(po_handle* h, HostRows& R, const DevBuf& dev, uint64_t n_rec, uint64_t nk, uint32_t k, uint32_t n_chunks,
                      double seen_share = 0.0) {
    if (nk == 0) return PO_OK;
    home::Pool* P = home::g_pool;
    PO_TRY(rows_room(h, R, nk, k, n_chunks, seen_share));
    const size_t elem = h->home_sh_b ? sizeof(uint64_t) : sizeof(po::Cand);
    const size_t bytes = (size_t)n_rec * elem;
    constexpr uint64_t N_EV = 32;   // flag words: slots 96 .. 127 of the landing zone
    if (h->home_used + bytes > h->home_stage.cap || (h->home_seq && h->home_seq % N_EV == 0)) {
        // the block is full (or every flag word has been used once): wait for the helper threads, start over at its beginning
        home_wait(h);
        if (hipStreamSynchronize(h->copy_stream) != hipSuccess) return fail(h, PO_ERR_HIP, "copy stream");
        h->home_used = 0;
        if (bytes > h->home_stage.cap)
            PO_TRY(ensure_host(h, h->home_stage, std::max<size_t>({bytes * 2, (size_t)(h->home_last_bytes + h->home_last_bytes / 8), (size_t)8 << 20})));
    }
    // behind the copy, on the same stream: a one-thread kernel writes a number into a page-locked word of the handle's landing
    // zone (slots 96 ..) -- what the pool's first thread polls
    const uint32_t slot = (uint32_t)(h->home_seq % N_EV);
    const uint32_t want = ++h->home_gen;
    char* dst = static_cast<char*>(h->home_stage.p) + h->home_used;
    // (Measured and not kept, round 4 -- profiles/r04_copy_kernels.txt.  Under the tracer the counting pass of the NEXT
    // piece shows 200-230 us instead of 90 while this copy is in flight (the runtime copies with a kernel of its own);
    // the HIP events of an untraced step do not (91 us per piece), and tools/copy_beside_kernel.py finds x 1.04-1.08.
    // A copy kernel of ours writing the page-locked block with 1 .. 256 workgroups: 5.1, 5.0, 5.1, 5.3, 5.4, 5.5 ms per step
    // against 4.7 -- the fewer waves the better, and the runtime's copy better than all of them; the same for the upload,
    // 6.8-7.8 ms.  Copying 50 % / 10 % of the bytes (timing only, the host reading the previous step's identical records):
    // 4.57 / 4.49 ms -- all of the interference is worth 0.2 ms, 8-byte records would buy 0.13.)
    HIP_TRY(h, hipMemcpyAsync(dst, dev.p, bytes, hipMemcpyDeviceToHost, h->copy_stream));
    hipLaunchKernelGGL(po::k_fill_u32, dim3(1), dim3(64), 0, h->copy_stream, reinterpret_cast<uint32_t*>(h->pinned_dev + 96 + slot), (uint64_t)1, want);
    HIP_TRY(h, hipGetLastError());
    home::Job j;
    j.rec = dst;
    j.sh_b = h->home_sh_b;
    j.sh_p = h->home_sh_p;
    j.n_rec = n_rec;
    j.out = static_cast<po_row*>(R.hb.p) + R.total;
    j.n_rows = nk;
    j.flag = reinterpret_cast<const volatile uint32_t*>(h->pinned + 96 + slot);
    j.want = want;
    j.paired = (h->bits == 2 && h->paired) ? 1u : 0u;
    j.bits = (uint32_t)h->bits;
    home::submit(P, j);
    ++h->home_seq;
    h->home_used += (bytes + 255) & ~size_t(255);
    h->home_last_bytes += bytes;
    R.total += nk;
    return PO_OK;
}

// rows of one chunk: room in the page-locked array, then the copy on the copy stream (dev must stay untouched
// until that stream has been synchronised)
po_status append_rows(po_handle* h, HostRows& R, const DevBuf& dev, uint64_t nk, uint32_t k, uint32_t n_chunks, double seen_share = 0.0) {
    if (nk == 0) return PO_OK;
    PO_TRY(rows_room(h, R, nk, k, n_chunks, seen_share));
    HIP_TRY(h, hipMemcpyAsync(static_cast<char*>(R.hb.p) + (size_t)R.total * sizeof(po_row), dev.p, (size_t)nk * sizeof(po_row),
                              hipMemcpyDeviceToHost, h->copy_stream));
    R.total += nk;
    return PO_OK;
}

void add_stats(po_stats& sum, const po_stats& S) {
    sum.n_candidates += S.n_candidates;
    sum.n_verified += S.n_verified;
    sum.n_rows += S.n_rows;
    sum.sum_overlap_bases += S.sum_overlap_bases;
    sum.verify_bytes_algo += S.verify_bytes_algo;
    sum.verify_bytes_exec += S.verify_bytes_exec;
    sum.n_tiles += S.n_tiles;
    sum.shard_bases += S.shard_bases;
    sum.fused_tail += S.fused_tail;
    sum.tail_fallback += S.tail_fallback;
    sum.n_predicted += S.n_predicted;
    sum.ms_index += S.ms_index;
    sum.ms_scan_count += S.ms_scan_count;
    sum.ms_scan_fill += S.ms_scan_fill;
    sum.ms_verify += S.ms_verify;
    sum.ms_select += S.ms_select;
    sum.ms_emit += S.ms_emit;
    sum.ms_total += S.ms_total;
    sum.ms_scan_probe += S.ms_scan_probe;
    sum.ms_verify_kernel += S.ms_verify_kernel;
}

// chunk k of a call emits into its own device buffer (kept on the handle): it must outlive its copy
po_status run_chunk(po_handle* h, const OverlapArgs& a, uint64_t* nk) {
    const uint32_t k = a.shard;
    po_result part;
    part.h = h;
    if (h->chunk_rows[k].p) {
        h->spare_rows.release();
        h->spare_rows = h->chunk_rows[k];
        h->chunk_rows[k] = DevBuf();
    }
    const po_status st = h->bits == 2 ? run_overlaps<2>(h, a, &part) : run_overlaps<8>(h, a, &part);
    h->chunk_rows[k] = part.d_rows;   // (run_overlaps returned: this chunk's rows are complete on the device)
    h->chunk_compact[k] = part.compact;
    part.d_rows = DevBuf();
    *nk = part.count;
    return st;
}

// May this call take the streamed form?
bool stream_eligible(const po_handle* h, uint32_t min_length) {
    const uint32_t n = (uint32_t)h->len.size();
    if (!h->dirty || h->bits != 2 || n < 4 || (n % 2) != 0 || !h->all_pairs_rcx) return false;
    if (h->asm_pieces) return false;
    if (getenv("PHASM_FULL_UPLOAD") || getenv("PHASM_NO_MIRROR")) return false;
    // (worth it from ~16 MB of packed even reads on: below that a piece's fixed cost, ~0.2 ms of small launches, is more
    // than the transfer time it hides)
    bool want = n >= 4096 && h->words[0].size() * 8 >= (16ull << 20);
    if (const char* e = getenv("PHASM_STREAM")) want = atoi(e) != 0;
    if (!want) return false;
    const uint32_t m = min_length ? min_length : 1;
    const uint64_t n_elig = count_eligible(const_cast<po_handle*>(h), m);
    if (n_elig == 0) return false;
    return true;   // (either index flavour: the narrow one needs every read's first word ahead of the pieces, the wide one two)
}

// piece boundaries (even read indices, first 0, last n): cut points in thousandths of the packed store.  Pair (a, b)
// can be computed once both reads are there, so the work released by a piece grows with its position -- the last
// pieces are made small, their rows are what is left to send home after the upload has ended.
std::vector<uint32_t> stream_bounds(const po_handle* h) {
    const uint32_t n = (uint32_t)h->len.size();
    // one piece per ~16 MB, 2 to 12 of them (8 until a piece's fixed device cost fell in round 3: config 2 5.18 -> 5.11 ms,
    // config 3 19.6 -> 19.0), cut at 1 - (1 - i/P)^1.25: 154/302/444/580/707/823/926 thousandths at P = 8
    // (config 2, 190 MB: 5.3 ms per step; 5 to 10 pieces measure within 3 % of it.  Config 2 scaled to 12 k reads, 45 MB:
    // 8 pieces 2.24 ms, 3 pieces 1.83, none 2.38; to 6 k reads, 22 MB: 8 pieces 1.74, 2 pieces 1.15, none 1.52)
    const uint64_t bytes0 = (uint64_t)h->words[0].size() * 8;
    // (the FIRST streamed call on a handle has no kept row buffers yet: every piece then costs two host round trips, and
    // eight pieces are the better cut -- 7.9 against 10.5 ms for the cold call at config 2)
    uint64_t max_pieces = h->chunk_rows[0].p ? 12 : 8;
    // (stores of half a gigabyte and more -- configs 3 and 5: a piece is milliseconds of device work there, its fixed cost is
    // nothing, and what counts is how little is left to do when the last byte has landed: 15 pieces, later ones smaller.
    // Config 3: 17.04 -> 16.59 ms; config 5, whose kernels take as long as its upload: 68.99 -> 68.77)
    const bool big = bytes0 >= (512ull << 20) && h->chunk_rows[0].p;
    if (big) max_pieces = 15;
    if (const char* e = getenv("PHASM_STREAM_MAX_PIECES")) max_pieces = (uint64_t)std::max(2, std::min(PO_MAX_PIECES - 1, atoi(e)));
    const uint32_t n_pieces = (uint32_t)std::min<uint64_t>(max_pieces, std::max<uint64_t>(2, (bytes0 + (8ull << 20)) / (16ull << 20)));
    const double skew = big ? 1.6 : 1.25;
    std::vector<uint32_t> cuts;
    for (uint32_t i = 1; i < n_pieces; ++i) cuts.push_back((uint32_t)(1000.0 * (1.0 - std::pow(1.0 - (double)i / n_pieces, skew))));
    if (const char* e = getenv("PHASM_STREAM_CUTS")) {
        cuts.clear();
        for (const char* q = e; *q;) {
            char* endp = nullptr;
            const long v = strtol(q, &endp, 10);
            if (endp == q) break;
            if (v > 0 && v < 1000 && (cuts.empty() || (uint32_t)v > cuts.back()) && cuts.size() + 1 < (size_t)PO_MAX_PIECES) cuts.push_back((uint32_t)v);
            q = *endp ? endp + 1 : endp;
        }
    }
    std::vector<uint32_t> b{0};
    const uint64_t total = h->words[0].size();
    for (uint32_t c : cuts) {
        const uint64_t target = total * c / 1000;
        uint32_t lo = 0, hi = n / 2;   // smallest pair i with woff[2 i] >= target
        while (lo < hi) {
            const uint32_t mid = (lo + hi) / 2;
            if (h->woff[2 * (size_t)mid] >= target) hi = mid; else lo = mid + 1;
        }
        if (2 * lo > b.back() && 2 * lo < n) b.push_back(2 * lo);
    }
    b.push_back(n);
    return b;
}

// start of a streamed step: everything but the packed words goes up, the pieces are queued on up_stream (one event
// each), every read's first word is put in place for the index
po_status stream_begin(po_handle* h, const std::vector<uint32_t>& bounds) {
    const uint32_t n = (uint32_t)h->len.size();
    const uint32_t P = (uint32_t)bounds.size() - 1;
    bool generate = false;
    if (!h->up_stream) HIP_TRY(h, hipStreamCreateWithFlags(&h->up_stream, hipStreamNonBlocking));
    for (uint32_t k = 0; k < P; ++k)
        if (!h->ev_piece[k]) HIP_TRY(h, hipEventCreate(&h->ev_piece[k]));
    auto queue_piece = [&](uint32_t k) -> po_status {
        uint64_t* dw = h->d_words.as<uint64_t>();
        const uint64_t wb = bounds[k] < n ? h->woff[bounds[k]] : h->words[0].size();
        const uint64_t we = bounds[k + 1] < n ? h->woff[bounds[k + 1]] : h->words[0].size();
        if (we > wb) {
            HIP_TRY(h, hipMemcpyAsync(dw + wb, h->words[0].data() + wb, (we - wb) * 8, hipMemcpyHostToDevice, h->up_stream));
            h->upload_bytes += (we - wb) * 8;
        }
        HIP_TRY(h, hipEventRecord(h->ev_piece[k], h->up_stream));
        return PO_OK;
    };
    // (Measured and not kept, round 4: the first piece on the wire BEFORE the step's preparation.  The per-read tables and the
    // first words are host->device copies too and queue behind the piece's 20 MB on the same engine, so the index -- built
    // from them while piece 0 is on the wire -- is late by what the piece takes to land.)
    PO_TRY(upload_meta(h, &generate));   // (sets upload_bytes to what the tables weigh)
    if (!generate) return fail(h, PO_ERR_INVALID, "streamed step on reads that are not (x, reverse complement of x) pairs");
    uint64_t* dw = h->d_words.as<uint64_t>();
    if (h->poison >= 0) {
        // (PHASM_POISON fills a fresh device buffer on the handle's stream: the pieces must not land under that fill)
        HIP_TRY(h, hipEventRecord(h->ev_up1, h->stream));
        HIP_TRY(h, hipStreamWaitEvent(h->up_stream, h->ev_up1, 0));
    }
    HIP_TRY(h, hipEventRecord(h->ev_up0, h->up_stream));
    PO_TRY(queue_piece(0));
    if (P > 1) {
        // first words of the reads of the later pieces (both strands: the host packed the odd store too, it just does
        // not travel), put in place on the handle's stream while piece 0 is crossing; the later pieces' copies are
        // ordered behind that kernel -- they bring the same values, but two writers of one word want an order
        // With the index built ahead of piece 0 (overlaps_streamed) the first words of piece 0's reads go up too: the index
        // build behind this kernel is then their only reader before the piece itself has landed, and the piece brings
        // the same values.
        const uint32_t r0 = h->st_early_index ? 0u : bounds[1];
        if (h->st_lead > 2) {
            // (large read sets: five words per read, so that the index can hold window minimisers -- 40 B per read ahead of
            // the pieces instead of 16, 2 % of the upload, for a counting pass of 0.55 x the time)
            note_lead_words(h);
            PO_TRY(ensure(h, h->d_first, (size_t)n * LEAD_WORDS * 8));
            HIP_TRY(h, hipMemcpyAsync(h->d_first.as<uint64_t>() + (size_t)LEAD_WORDS * r0, h->lead_words.data() + (size_t)LEAD_WORDS * r0,
                                      (size_t)(n - r0) * LEAD_WORDS * 8, hipMemcpyHostToDevice, h->stream));
            h->upload_bytes += (size_t)(n - r0) * LEAD_WORDS * 8;
            hipLaunchKernelGGL(po::k_scatter_lead, dim3(cdiv((uint64_t)(n - r0) * LEAD_WORDS, 256)), dim3(256), 0, h->stream, dw,
                               h->d_woff.as<uint64_t>(), h->d_len.as<uint32_t>(), h->d_first.as<uint64_t>(), LEAD_WORDS, r0, n);
        } else {
            note_first_words(h);   // (nothing to do when po_add_sequence kept them up to date)
            PO_TRY(ensure(h, h->d_first, (size_t)n * 16));
            HIP_TRY(h, hipMemcpyAsync(h->d_first.as<uint64_t>() + 2 * (size_t)r0, h->first_words.data() + 2 * (size_t)r0,
                                      (size_t)(n - r0) * 16, hipMemcpyHostToDevice, h->stream));
            h->upload_bytes += (size_t)(n - r0) * 16;
            hipLaunchKernelGGL(po::k_scatter_first, dim3(cdiv(n - r0, 256)), dim3(256), 0, h->stream, dw, h->d_woff.as<uint64_t>(),
                               h->d_first.as<ulonglong2>(), r0, n);
        }
        HIP_TRY(h, hipGetLastError());
        if (!h->ev_first) HIP_TRY(h, hipEventCreateWithFlags(&h->ev_first, hipEventDisableTiming));
        HIP_TRY(h, hipEventRecord(h->ev_first, h->stream));
        HIP_TRY(h, hipStreamWaitEvent(h->up_stream, h->ev_first, 0));
    }
    for (uint32_t k = 1; k < P; ++k) PO_TRY(queue_piece(k));
    HIP_TRY(h, hipEventRecord(h->ev_up1, h->up_stream));
    // reverse complements: piece k's odd reads as soon as piece k is there (needs the per-read tables of upload_meta and,
    // for the later pieces, the first words in place: both are on the handle's stream up to here)
    if (!h->rc_stream) HIP_TRY(h, hipStreamCreateWithFlags(&h->rc_stream, hipStreamNonBlocking));
    if (!h->ev_meta) HIP_TRY(h, hipEventCreateWithFlags(&h->ev_meta, hipEventDisableTiming));
    HIP_TRY(h, hipEventRecord(h->ev_meta, h->stream));
    HIP_TRY(h, hipStreamWaitEvent(h->rc_stream, h->ev_meta, 0));
    for (uint32_t k = 0; k < P; ++k) {
        if (!h->ev_rc[k]) HIP_TRY(h, hipEventCreateWithFlags(&h->ev_rc[k], hipEventDisableTiming));
        HIP_TRY(h, hipStreamWaitEvent(h->rc_stream, h->ev_piece[k], 0));
        const uint32_t p0 = bounds[k] / 2, p1 = bounds[k + 1] / 2;
        if (p1 > p0)
            hipLaunchKernelGGL(po::k_revcomp_store, dim3(cdiv((uint64_t)(p1 - p0) * 64, 256)), dim3(256), 0, h->rc_stream, dw,
                               h->d_woff.as<uint64_t>(), h->d_len.as<uint32_t>(), p0, p1,
                               h->n_exc_uploaded ? h->d_exc_off.as<uint32_t>() : nullptr, h->d_exc_pos.as<uint32_t>());
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipEventRecord(h->ev_rc[k], h->rc_stream));
    }
    // deferred containment list: [Cand x cap | counter]
    h->st_defer_cap = std::max<uint32_t>(1u << 16, h->defer_need + h->defer_need / 2);
    if (const char* e = getenv("PHASM_DEFER_CAP")) h->st_defer_cap = (uint32_t)std::max(1, atoi(e));   // (tests: force the overflow path)
    PO_TRY(ensure(h, h->d_defer, (size_t)h->st_defer_cap * sizeof(po::Cand) + 16));
    if (!getenv("PHASM_DEFER_CAP")) h->st_defer_cap = (uint32_t)std::min<size_t>((h->d_defer.cap - 16) / sizeof(po::Cand), 0xFFFFFF00u);
    HIP_TRY(h, hipMemsetAsync(h->d_defer.as<char>() + (size_t)h->st_defer_cap * sizeof(po::Cand), 0, 16, h->stream));
    h->paired = true;   // (checked on the host as the reads arrived: all_pairs_rcx)
    ++h->upload_gen;
    h->dirty = false;
    return PO_OK;
}

// The streamed step.  *overflow: the deferred list was too small (nothing was handed out; the reads are resident now,
// the caller takes the chunked form, and the next streamed call sizes the list by what this one counted).
po_status overlaps_streamed(po_handle* h, uint32_t min_length, HostRows& R, po_stats& sum, bool* overflow) {
    *overflow = false;
    const uint32_t n = (uint32_t)h->len.size();
    const std::vector<uint32_t> bounds = stream_bounds(h);
    const uint32_t P = (uint32_t)bounds.size() - 1;
    const bool trace = getenv("PHASM_STREAM_TRACE") != nullptr;   // developer aid: host-clock marks of the pipeline on stderr
    const auto t_start = std::chrono::steady_clock::now();
    auto since = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count(); };
    // the previous streamed call on the same reads, cuts and min_length tells how many candidates each piece will have
    std::vector<uint32_t> sig(bounds);
    sig.push_back(min_length);
    sig.push_back((uint32_t)(h->total_bases & 0xFFFFFFFFu));
    h->st_pred_valid = h->st_pred_valid && sig == h->st_pred_sig;
    uint64_t new_pred[PO_MAX_PIECES] = {};
    // the index ahead of piece 0: it needs every read's first word(s) only, and at 400 k reads (wide index, 2.9 ms; 16 ms at
    // 2 M reads) building it inside piece 0 -- after the piece has landed -- kept every later piece 2-3 ms behind its data
    h->st_selfclean = false;
    h->st_early_index = P > 1 && h->poison < 0 && !getenv("PHASM_NO_INDEX_REUSE") && !getenv("PHASM_LATE_INDEX");
    // words per read that travel ahead of the pieces: five where the pieces' index would use windows of 4 if it had them, else two
    h->st_lead = index_flavour(h, min_length ? min_length : 1, true, LEAD_WORDS, OverlapSwitches()).ww >= 4 && !getenv("PHASM_STREAM_LEAD2") ? LEAD_WORDS : 2u;
    PO_TRY(stream_begin(h, bounds));
    auto piece_args = [&](uint32_t k) {
        OverlapArgs a{min_length, k, P};
        a.streamed = true;
        a.r_begin = bounds[k];
        a.r_end = bounds[k + 1];
        return a;
    };
    if (trace) std::fprintf(stderr, "[stream] %u pieces queued at %.3f ms\n", P, since());
    if (h->st_early_index) {
        po_result part;
        part.h = h;
        OverlapArgs a = piece_args(0);
        a.idx_only = true;
        const po_status ist = run_overlaps<2>(h, a, &part);
        part.d_rows.release();
        if (ist != PO_OK) {
            (void)hipStreamSynchronize(h->stream);
            (void)hipStreamSynchronize(h->up_stream);
            (void)hipStreamSynchronize(h->rc_stream);
            h->dirty = true;
            return ist;
        }
    }
    uint64_t* dw = h->d_words.as<uint64_t>();
    po_status st = PO_OK;
    // a finished piece: statistics, rows queued for home.  Called by run_overlaps at the next piece's first host wait
    // (a piece that emitted into a buffer known to be large enough returns with its kernels still queued), or below.
    auto completed = [&](uint32_t k, const po_stats& S, uint64_t nk) -> po_status {
        add_stats(sum, S);
        new_pred[k] = S.n_candidates;
        const double seen = (double)bounds[k + 1] / (double)n;
        if (h->chunk_compact[k]) PO_TRY(append_home(h, R, h->chunk_rows[k], S.n_verified, nk, k, P, seen * seen));
        else PO_TRY(append_rows(h, R, h->chunk_rows[k], nk, k, P, seen * seen));
        if (trace) {
            float up = 0;
            (void)hipEventElapsedTime(&up, h->ev_up0, h->ev_piece[k]);
            std::fprintf(stderr, "[stream] piece %u reads [%u, %u): landed %.3f ms after the first copy started, rows counted at %.3f ms (device %.3f ms: scan %.3f verify %.3f), %llu rows (%.1f MB) queued for home\n",
                         k, bounds[k], bounds[k + 1], up, since(), S.ms_total, S.ms_scan_count + S.ms_scan_fill, S.ms_verify,
                         (unsigned long long)nk, nk * 24e-6);
        }
        return PO_OK;
    };
    h->st_pend.valid = false;
    bool tail_gave_up = false;   // a piece's k_tail met reads handed to the global (a, b) table (tandem repeats): chunked form
    h->st_harvest = [&]() -> po_status {
        const uint32_t k = h->st_pend.k;
        bool needs_classic = false;
        const uint64_t nk = finish_piece(h, &needs_classic);
        if (needs_classic) {
            tail_gave_up = true;
            return PO_OK;
        }
        return completed(k, h->st_pend.S, nk);
    };
    if (getenv("PHASM_STREAM_SYNC")) h->st_harvest = nullptr;   // (developer switch: every piece waits for its own end)
    for (uint32_t k = 0; k < P && st == PO_OK; ++k) {
        // piece k has landed and its odd reads (reverse complements) have been written next to it (rc_stream, stream_begin)
        if (hipStreamWaitEvent(h->stream, h->ev_rc[k], 0) != hipSuccess) { st = fail(h, PO_ERR_HIP, "hipStreamWaitEvent"); break; }
        OverlapArgs a = piece_args(k);
        // per-piece workspaces: sized for the largest piece when they are first needed.  A piece keeps the candidates
        // whose b lies below its a, so piece j has about (b[j+1]^2 - b[j]^2) / (b[k+1]^2 - b[k]^2) times piece k's
        {
            const double mine = (double)bounds[k + 1] * bounds[k + 1] - (double)bounds[k] * bounds[k];
            for (uint32_t j = k + 1; j < P; ++j)
                a.ws_scale = std::max(a.ws_scale, ((double)bounds[j + 1] * bounds[j + 1] - (double)bounds[j] * bounds[j]) / mine * 1.1);
        }
        h->ev = h->ev_sets[k & 1];
        uint64_t nk = 0;
        st = run_chunk(h, a, &nk);
        if (st != PO_OK || tail_gave_up) break;
        if (h->st_pend.valid && h->st_pend.k == k) continue;   // piece k is queued, its counts are read later (an older one was collected inside)
        if (h->st_pend.valid) {
            // (piece k never waited for the device -- it had nothing to scan: the older piece is still to be collected)
            if (hipStreamSynchronize(h->stream) != hipSuccess) { st = fail(h, PO_ERR_HIP, "stream"); break; }
            st = h->st_harvest();
            if (st != PO_OK) break;
        }
        st = completed(k, h->stats, nk);   // piece k waited for its own end
    }
    if (st == PO_OK && h->st_pend.valid && !tail_gave_up) {
        if (hipStreamSynchronize(h->stream) != hipSuccess) st = fail(h, PO_ERR_HIP, "stream");
        else st = h->st_harvest();
    }
    h->st_harvest = nullptr;
    h->st_pend.valid = false;
    h->ev = h->ev_sets[0];
    if (st == PO_OK && tail_gave_up) {
        // (rare: a read with hundreds of verified suffix-prefix hits.  Pieces may still be in flight and their odd reads
        // unwritten: everything is uploaded again by the chunked form)
        (void)hipStreamSynchronize(h->stream);
        (void)hipStreamSynchronize(h->up_stream);
        (void)hipStreamSynchronize(h->rc_stream);
        h->dirty = true;
        h->st_tail_gave_up = true;
        h->st_pred_valid = false;
        *overflow = true;
        return PO_OK;
    }
    if (st != PO_OK) {
        (void)hipStreamSynchronize(h->up_stream);
        (void)hipStreamSynchronize(h->rc_stream);
        h->dirty = true;   // (a piece may be missing on the device)
        h->st_pred_valid = false;
        return st;
    }
    h->st_pred_sig = sig;
    std::memcpy(h->st_pred_cand, new_pred, sizeof(new_pred));
    h->st_pred_valid = true;
    float ms = 0;
    (void)hipEventSynchronize(h->ev_up1);   // (recorded right behind the last piece's event, which the kernels waited for)
    (void)hipEventElapsedTime(&ms, h->ev_up0, h->ev_up1);
    h->stats.ms_upload = ms;
    // ---- the deferred containments: every read is there now
    HIP_TRY(h, hipMemcpyAsync(h->pinned + 40, h->d_defer.as<char>() + (size_t)h->st_defer_cap * sizeof(po::Cand), 8,
                              hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const uint32_t n_def = (uint32_t)h->pinned[40];
    h->defer_need = n_def;
    if (n_def > h->st_defer_cap) {
        *overflow = true;
        return PO_OK;
    }
    if (n_def) {
        hipStream_t s = h->stream;
        po::Cand* list = h->d_defer.as<po::Cand>();
        PO_TRY(ensure(h, h->d_rowcnt, (size_t)n_def));
        PO_TRY(ensure(h, h->d_row_off, ((size_t)n_def + 1) * 4));
        HIP_TRY(h, hipEventRecord(h->ev[EV_START], s));
        hipLaunchKernelGGL(po::k_verify_flat, dim3(cdiv((uint64_t)n_def * 64, 256)), dim3(256), 0, s, dw, h->d_woff.as<uint64_t>(),
                           h->d_len.as<uint32_t>(), list, n_def, h->n_exc_uploaded ? h->d_exc_off.as<uint32_t>() : nullptr,
                           h->d_exc_pos.as<uint32_t>(), h->d_exc_byte.as<uint8_t>());
        hipLaunchKernelGGL(po::k_deferred_rowcnt, dim3(cdiv(n_def, 256)), dim3(256), 0, s, list, n_def, 1u, h->d_rowcnt.as<uint8_t>());
        HIP_TRY(h, hipGetLastError());
        PO_TRY(prefix_sum<uint8_t>(h, h->d_rowcnt.as<uint8_t>(), n_def, h->d_row_off.as<uint32_t>(), &h->pinned[2]));
        HIP_TRY(h, hipStreamSynchronize(s));
        const uint64_t n_rows = h->pinned[2];
        if (n_rows) {
            PO_TRY(ensure(h, h->chunk_rows[P], n_rows * sizeof(po_row)));
            unsigned long long* scalars = h->d_scalars.as<unsigned long long>();
            HIP_TRY(h, hipMemsetAsync(scalars + 4, 0, 32, s));
            hipLaunchKernelGGL(po::k_emit_cands, dim3(std::min<uint32_t>(cdiv(n_def, 256), (uint32_t)h->n_cu * 16)), dim3(256), 0, s,
                               list, h->d_rowcnt.as<uint8_t>(), h->d_row_off.as<uint32_t>(), n_def, h->d_len.as<uint32_t>(),
                               h->chunk_rows[P].as<po::Row>(), 2u, 1u, scalars + 4);
            HIP_TRY(h, hipGetLastError());
            HIP_TRY(h, hipMemcpyAsync(h->pinned + 4, scalars + 4, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(h, hipEventRecord(h->ev[EV_EMIT], s));
            HIP_TRY(h, hipStreamSynchronize(s));
            float ms_def = 0;
            (void)hipEventElapsedTime(&ms_def, h->ev[EV_START], h->ev[EV_EMIT]);
            sum.n_verified += h->pinned[4];
            sum.sum_overlap_bases += h->pinned[5];
            sum.verify_bytes_algo += h->pinned[6];
            sum.verify_bytes_exec += h->pinned[7];
            sum.n_rows += n_rows;
            sum.ms_verify += ms_def;
            sum.ms_total += ms_def;
            PO_TRY(append_rows(h, R, h->chunk_rows[P], n_rows, P, P + 1));
        }
    }
    (void)n;
    if (trace) {
        std::fprintf(stderr, "[stream] deferred list settled at %.3f ms (%u candidates)\n", since(), n_def);
        (void)hipStreamSynchronize(h->copy_stream);
        std::fprintf(stderr, "[stream] last row home at %.3f ms\n", since());
    }
    return PO_OK;
}

}  // namespace
}  // extern "C++"

po_status po_overlaps_to_host(po_handle* h, uint32_t min_length, po_result** out) {
    if (!h || !out) return PO_ERR_INVALID;
    *out = nullptr;
    if (h->segments_only) return fail(h, PO_ERR_INVALID, "this handle holds GFA segments without sequences: nothing to overlap");
    // small jobs: nothing to overlap (a chunk costs ~40 kernel launches)
    uint32_t n_chunks = (h->len.size() >= 8192 && h->total_bases >= (64ull << 20)) ? 4u : 1u;
    if (const char* e = getenv("PHASM_HOST_CHUNKS")) n_chunks = (uint32_t)std::max(1, std::min(4, atoi(e)));
    po_result* r = new (std::nothrow) po_result();
    if (!r) return fail(h, PO_ERR_NOMEM, "out of host memory");
    r->h = h;
    po_status st = PO_OK;
    HostRows R;
    po_stats sum = {};
    bool streamed = false, overflowed = false;
    float ms_upload = 0;
    try {
        st = init_device(h);
        if (st == PO_OK && !h->copy_stream && hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking) != hipSuccess)
            st = fail(h, PO_ERR_HIP, "cannot create the copy stream");
        if (st == PO_OK && h->spare_host.p) {   // the pinned array of an earlier result, if there is one
            R.hb = h->spare_host;
            h->spare_host = HostBuf();
        }
        if (st == PO_OK) {
            (void)home_begin(h);   // rows home as records + helper threads (PHASM_HOME=0: every row crosses PCIe as before)
            h->home_last_bytes = 0;
        }
        if (st == PO_OK && stream_eligible(h, min_length)) {
            bool overflow = false;
            st = overlaps_streamed(h, min_length, R, sum, &overflow);
            ms_upload = h->stats.ms_upload;
            if (st == PO_OK && !overflow) {
                streamed = true;
            } else if (st == PO_OK) {
                // (rare: more containments of later reads than the list holds -- the reads are resident now)
                overflowed = true;
                home_wait(h);
                if (h->home_on) {   // (the abandoned step's records are not part of the result)
                    home::g_pool->sum_l.store(0);
                    home::g_pool->sum_b.store(0);
                    home::g_pool->sum_e.store(0);
                }
                if (hipStreamSynchronize(h->copy_stream) != hipSuccess) st = fail(h, PO_ERR_HIP, "copy stream");
                R.total = 0;
                sum = po_stats();
            }
        }
        if (st == PO_OK && !streamed) st = upload(h);
        for (uint32_t k = 0; k < n_chunks && st == PO_OK && !streamed; ++k) {
            uint64_t nk = 0;
            st = run_chunk(h, OverlapArgs{min_length, k, n_chunks}, &nk);
            if (st != PO_OK) break;
            add_stats(sum, h->stats);
            st = h->chunk_compact[k] ? append_home(h, R, h->chunk_rows[k], h->stats.n_verified, nk, k, n_chunks)
                                     : append_rows(h, R, h->chunk_rows[k], nk, k, n_chunks);
        }
    } catch (const std::bad_alloc&) {
        st = fail(h, PO_ERR_NOMEM, "out of host memory in po_overlaps_to_host");
    }
    h->st_harvest = nullptr;   // (an exception may have left the streamed step half way: its callback captures dead locals)
    h->st_pend.valid = false;
    h->ev = h->ev_sets[0];
    if (h->dev_ready) (void)hipStreamSynchronize(h->stream);
    if (h->up_stream) (void)hipStreamSynchronize(h->up_stream);
    if (h->rc_stream) (void)hipStreamSynchronize(h->rc_stream);
    if (h->copy_stream && hipStreamSynchronize(h->copy_stream) != hipSuccess && st == PO_OK) st = fail(h, PO_ERR_HIP, "row copy device->host");
    {
        // the helper threads have written every piece's rows before the array is handed out (or released)
        const int herr = home_end(h, &sum);
        if (herr && st == PO_OK)
            st = fail(h, PO_ERR_HIP, herr == 1 ? "internal: the host's row count of a piece differs from the device's"
                                     : herr == 2 ? "internal: a verified-candidate record names a read the handle does not hold"
                                                 : "the event behind a device->host copy of records failed");
    }
    if (st != PO_OK) {
        R.hb.release();
        delete r;
        return st;
    }
    // the call's statistics: sums over the chunks (per-call fields from the last chunk)
    po_stats& S = h->stats;
    S.n_candidates = sum.n_candidates;
    S.n_verified = sum.n_verified;
    S.n_rows = sum.n_rows;
    S.sum_overlap_bases = sum.sum_overlap_bases;
    S.verify_bytes_algo = sum.verify_bytes_algo;
    S.verify_bytes_exec = sum.verify_bytes_exec;
    S.n_tiles = sum.n_tiles;
    S.shard_bases = sum.shard_bases;
    S.ms_index = sum.ms_index;
    S.ms_scan_count = sum.ms_scan_count;
    S.ms_scan_fill = sum.ms_scan_fill;
    S.ms_verify = sum.ms_verify;
    S.ms_select = sum.ms_select;
    S.ms_emit = sum.ms_emit;
    S.ms_total = sum.ms_total;
    S.ms_scan_probe = sum.ms_scan_probe;
    S.ms_verify_kernel = sum.ms_verify_kernel;
    S.fused_tail = sum.fused_tail;
    S.n_predicted = sum.n_predicted;
    S.home_record_bytes = h->home_last_bytes ? (h->home_sh_b ? 8u : 16u) : 0u;
    S.tail_fallback = sum.tail_fallback + (h->st_tail_gave_up ? 1u : 0u);
    h->st_tail_gave_up = false;
    S.streamed = streamed ? 1u : 0u;
    S.n_deferred = (streamed || overflowed) ? h->defer_need : 0u;   // (streamed == 0 with n_deferred > 0: the list overflowed, chunked form taken)
    if (streamed) {
        S.ms_upload = ms_upload;
        S.upload_bytes = h->upload_bytes;
    }
    h->last_host_rows = R.total;
    r->count = R.total;
    r->unique_twins = h->bits == 2 && h->paired;   // (chunks are a-major and disjoint in a: groups stay adjacent)
    if (R.total) {
        r->host = R.hb.p;
        r->host_cap = R.hb.cap;
    } else if (R.hb.p) {
        h->spare_host = R.hb;   // nothing to hand out: keep the buffer
    }
    ++h->live_results;
    *out = r;
    return PO_OK;
}

// ---- sliced wide index for multi-GPU steps (phasm_amd/dist.py: IndexExchange) ------------------------------------
po_status po_index_slice_build(po_handle* h, uint32_t min_length, uint32_t slice, uint32_t n_slices, uint32_t* is_wide,
                               uint32_t* slice_bits, uint64_t* chain_entries) {
    if (!h || !is_wide || !slice_bits || !chain_entries) return PO_ERR_INVALID;
    if (n_slices < 2 || slice >= n_slices) return fail(h, PO_ERR_INVALID, "po_index_slice_build: need 2 or more slices and slice < n_slices");
    *is_wide = 0;
    *slice_bits = 0;
    *chain_entries = 0;
    OverlapArgs a{min_length};
    a.build_slice = slice;
    a.build_n = n_slices;
    h->sl_is_wide = false;
    po_result* r = nullptr;
    const po_status st = overlaps_common(h, a, &r);
    if (r) po_result_free(r);
    if (st != PO_OK) return st;
    *is_wide = h->sl_is_wide ? 1u : 0u;
    if (h->sl_is_wide) {
        *slice_bits = h->sl_tbits;
        *chain_entries = h->sl_entries;
    }
    return PO_OK;
}

// the triple a caller hands to the *_indexed entry points describes a buffer the library cannot see: refuse what cannot
// be a sliced index at all (a shift by slice_bits >= 64 is undefined, the scan addresses 2^slice_bits slots per chunk)
static bool slice_args_ok(uint32_t n_slices, uint32_t slice_bits, uint64_t chain_capacity) {
    return n_slices >= 2 && n_slices <= 4096 && slice_bits >= 1 && slice_bits <= 30 && chain_capacity < (1ull << 36);
}

uint64_t po_index_chunk_bytes(uint32_t slice_bits, uint64_t chain_capacity, uint64_t* chain_offset_bytes) {
    if (chain_offset_bytes) *chain_offset_bytes = 0;
    if (slice_bits < 1 || slice_bits > 30 || chain_capacity >= (1ull << 36)) return 0;   // (not a sliced index)
    // [2^bits + 1 slots of 16 bytes | padding to 256 | chain_capacity entries of 8 bytes | padding to 256]
    const uint64_t off = ((((1ull << slice_bits) + 1ull) * sizeof(po::Slot)) + 255ull) & ~255ull;
    if (chain_offset_bytes) *chain_offset_bytes = off;
    return (off + chain_capacity * 8ull + 255ull) & ~255ull;
}

// the gathered index of an *_indexed call as run_overlaps wants it described
static po_status indexed_args(po_handle* h, const void* index_device, uint32_t n_slices, uint32_t slice_bits, uint64_t chain_capacity,
                              OverlapArgs* a) {
    uint64_t off = 0;
    const uint64_t chunk = po_index_chunk_bytes(slice_bits, chain_capacity, &off);
    if ((chunk / 16) * n_slices >= 0xFFFFFFF0ull) return fail(h, PO_ERR_CAPACITY, "sliced index larger than 64 GB");
    a->ext_index = index_device;
    a->ext_slices = n_slices;
    a->ext_tbits = slice_bits;
    a->ext_chunk_slots = (uint32_t)(chunk / 16);
    a->ext_chain_off = (uint32_t)(off / 16);
    return PO_OK;
}

po_status po_index_slice_export(po_handle* h, void* dst_device, uint64_t chain_capacity) {
    if (!h || !dst_device) return PO_ERR_INVALID;
    if (!h->sl_is_wide || !h->dev_ready) return fail(h, PO_ERR_INVALID, "po_index_slice_export: no sub-table has been built on this handle");
    if (chain_capacity < h->sl_entries) return fail(h, PO_ERR_INVALID, "po_index_slice_export: chain capacity below this sub-table's entries");
    uint64_t off = 0;
    (void)po_index_chunk_bytes(h->sl_tbits, chain_capacity, &off);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpyAsync(dst_device, h->d_table.p, ((size_t)(1ull << h->sl_tbits) + 1) * sizeof(po::Slot), hipMemcpyDeviceToDevice, h->stream));
    if (h->sl_entries)
        HIP_TRY(h, hipMemcpyAsync(static_cast<char*>(dst_device) + off, h->d_chain.p, (size_t)h->sl_entries * 8, hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return PO_OK;
}

po_status po_candidates_shard_indexed(po_handle* h, uint32_t min_length, uint32_t shard, uint32_t nshards,
                                      const void* index_device, uint32_t n_slices, uint32_t slice_bits, uint64_t chain_capacity,
                                      void* dst_device, uint64_t capacity, int* written, po_result** out) {
    if (written) *written = 0;
    if (!h || !out || !index_device) return PO_ERR_INVALID;
    if (!slice_args_ok(n_slices, slice_bits, chain_capacity))
        return fail(h, PO_ERR_INVALID, "sliced index: need 2..4096 slices of 2^1..2^30 slots (slice_bits as po_index_slice_build reported it)");
    if (!dst_device && capacity) return PO_ERR_INVALID;
    OverlapArgs a{min_length, shard, nshards, true};
    PO_TRY(indexed_args(h, index_device, n_slices, slice_bits, chain_capacity, &a));
    const po_status st = overlaps_common(h, a, out, dst_device, capacity);
    if (st == PO_OK && written) *written = (*out)->wrote_ext ? 1 : 0;
    return st;
}

// (test hook: the row form of the same call)
po_status po_overlaps_shard_indexed(po_handle* h, uint32_t min_length, uint32_t shard, uint32_t nshards, const void* index_device,
                                    uint32_t n_slices, uint32_t slice_bits, uint64_t chain_capacity, po_result** out) {
    if (!h || !out || !index_device) return PO_ERR_INVALID;
    if (!slice_args_ok(n_slices, slice_bits, chain_capacity))
        return fail(h, PO_ERR_INVALID, "sliced index: need 2..4096 slices of 2^1..2^30 slots (slice_bits as po_index_slice_build reported it)");
    OverlapArgs a{min_length, shard, nshards, false};
    PO_TRY(indexed_args(h, index_device, n_slices, slice_bits, chain_capacity, &a));
    return overlaps_common(h, a, out);
}

po_status po_overlaps_ex(po_handle* h, uint32_t min_length, uint32_t max_diff, uint32_t band, po_result** out) {
    if (!h || !out) return PO_ERR_INVALID;
    *out = nullptr;
    if (band > 30) return fail(h, PO_ERR_INVALID, "po_overlaps_ex: band must be <= 30 (2*band+1 diagonals on lanes 1..61, one lane each; lanes 0 and 63 let the bases in)");
    if (max_diff >= (1u << 16)) return fail(h, PO_ERR_INVALID, "po_overlaps_ex: max_diff must be < 65536");
    OverlapArgs a{min_length};
    a.dp = true;
    a.dp_E = max_diff;
    a.dp_W = band;
    return overlaps_common(h, a, out);
}

po_status po_shard_range(const po_handle* h, uint32_t shard, uint32_t nshards, uint32_t* r_begin, uint32_t* r_end) {
    if (!h || !r_begin || !r_end || nshards == 0 || shard >= nshards) return PO_ERR_INVALID;
    try {
        shard_range(h, shard, nshards, r_begin, r_end, nullptr);
    } catch (const std::bad_alloc&) {
        return PO_ERR_NOMEM;
    }
    return PO_OK;
}

uint64_t po_result_count(const po_result* r) { return r ? r->count : 0; }

const po_row* po_result_rows(po_result* r) {
    if (!r) return nullptr;
    if (r->host || r->count == 0) return static_cast<const po_row*>(r->host);
    po_handle* h = r->h;
    const void* src = r->wrote_ext ? r->ext_dst : r->d_rows.p;  // (wrote_ext: the entries live in the caller's buffer)
    if (!src) return nullptr;
    if (hipSetDevice(h->device) != hipSuccess) return nullptr;
    // the destination is pinned memory owned by the handle's pool: one DMA at the PCIe rate, and no pageable
    // heap range is ever handed to the runtime as a copy target
    const size_t bytes = r->count * r->elem;
    HostBuf hb;
    if (h->spare_host.cap >= bytes) {
        hb = h->spare_host;
        h->spare_host = HostBuf();
    } else if (ensure_host(h, hb, bytes) != PO_OK) {
        return nullptr;
    }
    hipError_t e = hipMemcpyAsync(hb.p, src, bytes, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(h->stream);
        fail(h, PO_ERR_HIP, std::string("row copy device->host: ") + hipGetErrorString(e));
        hb.release();
        return nullptr;
    }
    r->host = hb.p;
    r->host_cap = hb.cap;
    return static_cast<const po_row*>(r->host);
}

// Rows [first, first + count) only: what ONE rank of a multi-GPU job brings home -- every rank holds the merged rows
// on its device, the ranks' hosts (one node) together receive them once.
const po_row* po_result_rows_range(po_result* r, uint64_t first, uint64_t count) {
    if (!r || first > r->count || count > r->count - first) return nullptr;
    if (count == 0) return nullptr;
    if (r->host) return reinterpret_cast<const po_row*>(static_cast<const char*>(r->host) + first * r->elem);
    po_handle* h = r->h;
    const char* src = static_cast<const char*>(r->wrote_ext ? r->ext_dst : r->d_rows.p);
    if (!src || hipSetDevice(h->device) != hipSuccess) return nullptr;
    const size_t bytes = count * r->elem;
    if (ensure_host(h, h->scratch_host, bytes) != PO_OK) return nullptr;
    hipError_t e = hipMemcpyAsync(h->scratch_host.p, src + first * r->elem, bytes, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(h->stream);
        fail(h, PO_ERR_HIP, std::string("row copy device->host: ") + hipGetErrorString(e));
        return nullptr;
    }
    return static_cast<const po_row*>(h->scratch_host.p);   // (valid until the next call that uses the handle's scratch)
}

const void* po_result_device_rows(const po_result* r) { return r ? (r->wrote_ext ? r->ext_dst : r->d_rows.p) : nullptr; }

po_status po_result_copy_to_device(po_result* r, void* dst_device) {
    if (!r || (!dst_device && r->count)) return PO_ERR_INVALID;
    if (r->count == 0) return PO_OK;
    po_handle* h = r->h;
    PO_TRY(init_device(h));
    PO_TRY(rows_to_device(h, r));
    HIP_TRY(h, hipMemcpyAsync(dst_device, r->d_rows.p, r->count * r->elem, hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return PO_OK;
}

po_status po_result_copy_prefix_to_device(po_result* r, void* dst_device, uint64_t count) {
    if (!r || (!dst_device && count)) return PO_ERR_INVALID;
    if (count > r->count) return fail(r->h, PO_ERR_INVALID, "po_result_copy_prefix_to_device: count exceeds the result");
    if (count == 0) return PO_OK;
    po_handle* h = r->h;
    PO_TRY(init_device(h));
    PO_TRY(rows_to_device(h, r));
    HIP_TRY(h, hipMemcpyAsync(dst_device, r->d_rows.p, count * r->elem, hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return PO_OK;
}

void po_result_free(po_result* r) {
    if (!r) return;
    po_handle* h = r->h;
    if (r->host_malloced) {
        std::free(r->host);
    } else if (r->host) {
        HostBuf hb;
        hb.p = r->host;
        hb.cap = r->host_cap;
        if (h && hb.cap > h->spare_host.cap) {  // keep the larger pinned buffer for the next result
            h->spare_host.release();
            h->spare_host = hb;
        } else {
            hb.release();
        }
    }
    r->host = nullptr;
    if (h) {
        --h->live_results;
        // keep the larger buffer for the next call
        DevBuf* spare = r->special == 3 ? &h->spare_spell
                        : r->elem == sizeof(po_row) ? &h->spare_rows : (r->kind_edges ? &h->spare_edges : &h->spare_cands);
        if (r->d_rows.p && r->d_rows.cap > spare->cap) {
            spare->release();
            *spare = r->d_rows;
            r->d_rows = DevBuf();
        }
    }
    if (h && r->d_nrank.p && r->d_nrank.cap > h->spare_nrank.cap) {
        h->spare_nrank.release();
        h->spare_nrank = r->d_nrank;
        r->d_nrank = DevBuf();
    }
    release_device(r);
    delete r;
}

// GFA2 edge lines for every row, byte-identical to the reference's
// gfa_line("E", "*", a_id, b_id, astart, aend, bstart, bend, "*")  (assembler.py:46-48, gfa.py:230-231).
po_status po_write_gfa_edges(po_result* r, int fd, uint64_t* lines_out) {
    if (!r || fd < 0) return PO_ERR_INVALID;
    po_handle* h = r->h;
    const bool graph_edges = r->elem == sizeof(po_edge);  // a po_layout_edges result: gfa2_write_graph's E lines
    if (r->elem != sizeof(po_row) && !graph_edges) return fail(h, PO_ERR_INVALID, "po_write_gfa_edges needs a row or edge result");
    if (lines_out) *lines_out = 0;
    if (r->count == 0) return PO_OK;
    const po_row* rows = po_result_rows(r);
    if (!rows) return PO_ERR_HIP;
    // Formatting 7 M lines and copying 324 MB into the file are the long parts of the `overlap` command after the call
    // itself (0.3-0.4 s at config 2 with a dozen threads appending to std::string and ONE thread writing).  Now: chunks of
    // 32 k rows are handed out dynamically to up to 16 threads; a thread formats its chunk straight into a buffer sized for
    // the worst case (two ids + four integers per line, digits from a two-digit table), learns its file offset from the
    // chunk before it (offsets are published along the chain as the sizes become known) and writes its own bytes with
    // pwrite -- formatting and the copy into the page cache both run in parallel, the file's bytes are the same.  A
    // descriptor that cannot seek (a pipe) keeps the ordered write() of whole chunks.
    size_t max_id = 0;
    for (const std::string& id : h->ids) max_id = std::max(max_id, id.size());
    const uint64_t chunk = 1u << 15;
    const uint64_t n_chunks = (r->count + chunk - 1) / chunk;
    const size_t line_max = 2 * max_id + 4 * 11 + 16;
    const off_t base_off = ::lseek(fd, 0, SEEK_CUR);
    // pwrite at a computed offset needs a regular file that honours the offset: on an O_APPEND descriptor Linux ignores it
    // and appends, so the chunks would land in the order the threads finish (`>> out.gfa`, a file opened in mode "a");
    // lseek also succeeds on descriptors that are no files at all.  Those take the ordered write() like a pipe.
    struct stat fd_st;
    const int fd_fl = ::fcntl(fd, F_GETFL);
    const bool seekable = base_off >= 0 && fd_fl >= 0 && !(fd_fl & O_APPEND) && ::fstat(fd, &fd_st) == 0 && S_ISREG(fd_st.st_mode);
    static const char digits2[201] =
        "00010203040506070809101112131415161718192021222324252627282930313233343536373839404142434445464748495051525354555657585960616263646566676869707172737475767778798081828384858687888990919293949596979899";
    auto put_int = [&](char* q, long long v) -> char* {
        if (v < 0) {
            *q++ = '-';
            v = -v;
        }
        unsigned long long u = (unsigned long long)v;
        char tmp[24];
        int n = 0;
        while (u >= 100) {
            const unsigned d = (unsigned)(u % 100) * 2;
            u /= 100;
            tmp[n++] = digits2[d + 1];
            tmp[n++] = digits2[d];
        }
        if (u >= 10) {
            tmp[n++] = digits2[u * 2 + 1];
            tmp[n++] = digits2[u * 2];
        } else {
            tmp[n++] = (char)('0' + u);
        }
        while (n) *q++ = tmp[--n];
        return q;
    };
    // one chunk -> buf; returns the bytes written, or -1 when a row names an unknown read
    auto format_chunk = [&](uint64_t lo, uint64_t hi, char* buf) -> long long {
        char* q = buf;
        const size_t n_ids = h->ids.size();
        for (uint64_t i = lo; i < hi; ++i) {
            po_row x;
            if (graph_edges) {
                // E * u v weight len(u) 0 overlap_len *   (gfa2_write_graph, phasm/io/gfa.py:315-327)
                const po_edge& e = reinterpret_cast<const po_edge*>(rows)[i];
                if (e.u >= n_ids || e.v >= n_ids) return -1;
                x = po_row{e.u, e.v, e.weight, (int32_t)h->len[e.u], 0, e.overlap_len};
            } else {
                x = rows[i];
            }
            if (x.a_idx >= n_ids || x.b_idx >= n_ids) return -1;
            const std::string &ia = h->ids[x.a_idx], &ib = h->ids[x.b_idx];
            std::memcpy(q, "E\t*\t", 4);
            q += 4;
            std::memcpy(q, ia.data(), ia.size());
            q += ia.size();
            *q++ = '\t';
            std::memcpy(q, ib.data(), ib.size());
            q += ib.size();
            *q++ = '\t';
            q = put_int(q, x.astart);
            *q++ = '\t';
            q = put_int(q, x.aend);
            *q++ = '\t';
            q = put_int(q, x.bstart);
            *q++ = '\t';
            q = put_int(q, x.bend);
            std::memcpy(q, "\t*\n", 3);
            q += 3;
        }
        return (long long)(q - buf);
    };
    try {
        const unsigned hw = cpu_share();
        const unsigned n_thr = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(std::min<unsigned>(hw, 16), n_chunks));
        // off[c] = file offset of chunk c (-1 until chunk c - 1 has been formatted); off[n_chunks] = the end
        std::unique_ptr<std::atomic<long long>[]> off(new std::atomic<long long>[n_chunks + 1]);
        for (uint64_t c = 0; c <= n_chunks; ++c) off[c].store(-1, std::memory_order_relaxed);
        off[0].store(seekable ? (long long)base_off : 0);
        std::atomic<uint64_t> next{0};
        std::atomic<int> failed{0};   // 1 unknown read, 2 write error, 3 out of memory
        // a pipe: chunk c may only be written once chunk c - 1 has been (written[c] = done)
        std::unique_ptr<std::atomic<int>[]> written(new std::atomic<int>[n_chunks + 1]);
        for (uint64_t c = 0; c <= n_chunks; ++c) written[c].store(c == 0 ? 1 : 0, std::memory_order_relaxed);
        auto work = [&]() {
            std::unique_ptr<char[]> buf;
            try {
                buf.reset(new char[(size_t)chunk * line_max]);
            } catch (const std::bad_alloc&) {
                failed.store(3);
            }
            for (;;) {
                const uint64_t c = next.fetch_add(1);
                if (c >= n_chunks) return;
                long long n = -1;
                if (!failed.load()) {
                    n = format_chunk(c * chunk, std::min<uint64_t>(r->count, (c + 1) * chunk), buf.get());
                    if (n < 0) failed.store(1);
                }
                // (the chain of offsets goes on even after a failure: nobody may wait for ever)
                long long at;
                while ((at = off[c].load(std::memory_order_acquire)) < 0) home::cpu_pause();
                off[c + 1].store(at + std::max<long long>(n, 0), std::memory_order_release);
                if (!seekable)
                    while (!written[c].load(std::memory_order_acquire)) home::cpu_pause();
                if (n > 0 && !failed.load()) {
                    const char* p = buf.get();
                    long long left = n, pos = at;
                    while (left) {
                        const ssize_t w = seekable ? ::pwrite(fd, p, (size_t)left, (off_t)pos) : ::write(fd, p, (size_t)left);
                        if (w < 0) {
                            failed.store(2);
                            break;
                        }
                        p += w;
                        pos += w;
                        left -= w;
                    }
                }
                if (!seekable) written[c + 1].store(1, std::memory_order_release);
            }
        };
        std::vector<std::thread> thr;
        try {
            for (unsigned t = 1; t < n_thr; ++t) thr.emplace_back(work);
        } catch (const std::system_error&) {
            // fewer threads than asked for: carry on with those that started
        }
        work();
        for (auto& th : thr) th.join();
        if (failed.load() == 1) return fail(h, PO_ERR_INVALID, "a row names an unknown read");
        if (failed.load() == 2) return fail(h, PO_ERR_INVALID, "write failed");
        if (failed.load() == 3) return fail(h, PO_ERR_NOMEM, "out of host memory");
        if (seekable && ::lseek(fd, (off_t)off[n_chunks].load(), SEEK_SET) < 0) return fail(h, PO_ERR_INVALID, "lseek failed");
    } catch (const std::bad_alloc&) {
        return fail(h, PO_ERR_NOMEM, "out of host memory");
    }
    if (lines_out) *lines_out = r->count;
    return PO_OK;
}


// `S <name> <length> *` for every read pair (x+, x-) of the handle, the way the overlap command writes them
// before the E lines (assembler.py:38)
po_status po_write_gfa_segments(po_handle* h, int fd, uint64_t* lines_out) {
    if (!h || fd < 0) return PO_ERR_INVALID;
    if (lines_out) *lines_out = 0;
    if (!ids_are_strand_pairs(h)) return fail(h, PO_ERR_INVALID, "po_write_gfa_segments needs reads added as name+\"+\" / name+\"-\" pairs");
    try {
        std::string buf;
        buf.reserve(1 << 20);
        for (size_t i = 0; i < h->ids.size(); i += 2) {
            buf.append("S\t");
            buf.append(h->ids[i], 0, h->ids[i].size() - 1);
            buf.push_back('\t');
            buf.append(std::to_string(h->len[i]));
            buf.append("\t*\n");
        }
        const char* p = buf.data();
        size_t left = buf.size();
        while (left) {
            ssize_t w = ::write(fd, p, left);
            if (w < 0) return fail(h, PO_ERR_INVALID, "write failed");
            p += w;
            left -= (size_t)w;
        }
    } catch (const std::bad_alloc&) {
        return fail(h, PO_ERR_NOMEM, "out of host memory");
    }
    if (lines_out) *lines_out = h->ids.size() / 2;
    return PO_OK;
}

po_status po_add_segment(po_handle* h, const char* name, size_t name_len, uint32_t length) {
    if (!h || (!name && name_len)) return PO_ERR_INVALID;
    try {
        return add_segment(h, name, name_len, length);
    } catch (const std::bad_alloc&) {
        return fail(h, PO_ERR_NOMEM, "out of host memory in po_add_segment");
    }
}

po_status po_result_from_rows(po_handle* h, const po_row* rows, uint64_t n, po_result** out) {
    if (!h || !out || (!rows && n)) return PO_ERR_INVALID;
    *out = nullptr;
    po_result* r = new (std::nothrow) po_result();
    if (!r) return fail(h, PO_ERR_NOMEM, "out of host memory");
    r->h = h;
    r->count = n;
    if (n) {
        r->host = std::malloc(n * sizeof(po_row));
        if (!r->host) {
            delete r;
            return fail(h, PO_ERR_NOMEM, "out of host memory for the row array");
        }
        std::memcpy(r->host, rows, n * sizeof(po_row));
        r->host_malloced = true;
    }
    ++h->live_results;
    *out = r;
    return PO_OK;
}

po_status po_add_gfa(po_handle* h, const char* path, uint64_t* n_segments, po_result** rows_out) {
    if (!h || !path || !rows_out) return PO_ERR_INVALID;
    *rows_out = nullptr;
    if (n_segments) *n_segments = 0;
    if (!h->len.empty()) return fail(h, PO_ERR_INVALID, "po_add_gfa needs an empty handle");
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0) return fail(h, PO_ERR_INVALID, std::string("cannot open ") + path);
    struct stat sb;
    if (::fstat(fd, &sb) != 0) {
        ::close(fd);
        return fail(h, PO_ERR_INVALID, std::string("cannot stat ") + path);
    }
    const size_t size = (size_t)sb.st_size;
    const char* data = nullptr;
    if (size) {
        void* m = ::mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m == MAP_FAILED) {
            ::close(fd);
            return fail(h, PO_ERR_INVALID, std::string("cannot map ") + path);
        }
        data = static_cast<const char*>(m);
    }
    po_status st = PO_OK;
    std::vector<po_row> rows;
    try {
        // every line of the file, '\n'-terminated (a '\r' before it is white space to strip())
        auto for_lines = [&](char tag, auto&& fn) {
            size_t pos = 0;
            while (pos < size && st == PO_OK) {
                const char* nl = static_cast<const char*>(std::memchr(data + pos, '\n', size - pos));
                const size_t len = nl ? (size_t)(nl - (data + pos)) : size - pos;
                if (len && data[pos] == tag) fn(data + pos, len);
                pos += len + 1;
            }
        };
        // pass 1: segments (gfa2_segment_to_read, gfa.py:33-46)
        NameIndex idx;
        std::vector<std::pair<std::string, uint32_t>> segs;
        std::unordered_map<std::string, size_t> seen;
        for_lines('S', [&](const char* p, size_t n) {
            Field f[4];
            long long length = 0;
            if (split_tabs(p, n, f, 4) < 4 || !parse_int(f[2], false, length) || length < 0 || length > 0x7FFFFFF0ll) {
                st = fail(h, PO_ERR_INVALID, "malformed GFA2 segment line: " + std::string(p, std::min<size_t>(n, 80)));
                return;
            }
            strip(f[1].p, f[1].n);
            std::string name(f[1].p, f[1].n);
            auto it = seen.find(name);
            if (it != seen.end()) {
                segs[it->second].second = (uint32_t)length;  // dict semantics: one entry per name, the last length wins (gfa.py:109)
            } else {
                seen.emplace(name, segs.size());
                segs.emplace_back(std::move(name), (uint32_t)length);
            }
        });
        seen.clear();
        if (st == PO_OK) {
            for (auto& sgm : segs) {
                if ((st = add_segment(h, sgm.first.data(), sgm.first.size(), sgm.second)) != PO_OK) break;
            }
        }
        if (st == PO_OK) idx.build(h);
        if (n_segments) *n_segments = segs.size();
        segs.clear();
        segs.shrink_to_fit();
        // pass 2: edges (gfa2_parse_edge, gfa.py:72-87; gfa2_line_to_la, :90-104).  The file is cut into byte ranges
        // at line starts and a few threads parse one range each (7 M lines: 0.4 s on one core at config 2); the
        // per-range row vectors are joined in file order, the first error in file order wins.
        struct Part {
            std::vector<po_row> rows;
            std::string err;
        };
        auto parse_range = [&](size_t lo, size_t hi, Part& out) {
            const char* last_a = nullptr;
            size_t last_a_n = 0;
            long last_a_idx = -1;
            auto node_of = [&](Field f, bool cache) -> long {
                strip(f.p, f.n);
                if (f.n < 1) return -1;
                const char strand = f.p[f.n - 1];
                if (strand != '+' && strand != '-') return -1;
                long r;
                if (cache && last_a && last_a_n == f.n - 1 && std::memcmp(last_a, f.p, f.n - 1) == 0) {
                    r = last_a_idx;
                } else {
                    r = idx.find(h, f.p, f.n - 1);
                    if (cache) last_a = f.p, last_a_n = f.n - 1, last_a_idx = r;
                }
                return r < 0 ? -1 : 2 * r + (strand == '-');
            };
            size_t pos = lo;
            while (pos < hi) {
                const char* nl = static_cast<const char*>(std::memchr(data + pos, '\n', size - pos));
                const size_t n = nl ? (size_t)(nl - (data + pos)) : size - pos;
                const char* p = data + pos;
                pos += n + 1;
                if (!n || p[0] != 'E') continue;
                Field f[9];
                long long v[4];
                if (split_tabs(p, n, f, 9) < 9 || !parse_int(f[4], true, v[0]) || !parse_int(f[5], true, v[1]) ||
                    !parse_int(f[6], true, v[2]) || !parse_int(f[7], true, v[3])) {
                    out.err = "malformed GFA2 edge line: " + std::string(p, std::min<size_t>(n, 80));
                    return;
                }
                const long a = node_of(f[2], true), b = node_of(f[3], false);
                if (a < 0 || b < 0) {
                    out.err = "GFA2 edge names an unknown segment or strand: " + std::string(p, std::min<size_t>(n, 80));
                    return;
                }
                for (long long x : v)
                    if (x < -0x7FFFFFFFll || x > 0x7FFFFFFFll) {
                        out.err = "GFA2 edge position out of range";
                        return;
                    }
                out.rows.push_back(po_row{(uint32_t)a, (uint32_t)b, (int32_t)v[0], (int32_t)v[1], (int32_t)v[2], (int32_t)v[3]});
            }
        };
        if (st == PO_OK && size) {
            const unsigned hw = cpu_share();
            const unsigned n_parts = (unsigned)std::max<size_t>(1, std::min<size_t>(std::min(hw, 12u), size >> 22));
            std::vector<size_t> cut(n_parts + 1, size);
            cut[0] = 0;
            for (unsigned k = 1; k < n_parts; ++k) {  // a range starts right after a newline
                size_t c = size / n_parts * k;
                const char* nl = static_cast<const char*>(std::memchr(data + c, '\n', size - c));
                cut[k] = nl ? (size_t)(nl - data) + 1 : size;
            }
            std::vector<Part> parts(n_parts);
            std::vector<std::thread> thr;
            std::atomic<int> oom{0};
            auto run = [&](unsigned k) {
                try {
                    parse_range(cut[k], cut[k + 1], parts[k]);
                } catch (...) {
                    oom.store(1);
                }
            };
            try {
                for (unsigned k = 1; k < n_parts; ++k) thr.emplace_back(run, k);
            } catch (const std::system_error&) {
            }
            const unsigned started = (unsigned)thr.size() + 1;
            run(0);
            for (auto& th : thr) th.join();
            for (unsigned k = started; k < n_parts; ++k) run(k);  // (threads that could not be started)
            if (oom.load()) throw std::bad_alloc();
            size_t total = 0;
            for (const Part& pt : parts) {
                if (!pt.err.empty()) {
                    st = fail(h, PO_ERR_INVALID, pt.err);
                    break;
                }
                total += pt.rows.size();
            }
            if (st == PO_OK) {
                rows.reserve(total);
                for (Part& pt : parts) {
                    rows.insert(rows.end(), pt.rows.begin(), pt.rows.end());
                    std::vector<po_row>().swap(pt.rows);
                }
            }
        }
    } catch (const std::bad_alloc&) {
        st = fail(h, PO_ERR_NOMEM, "out of host memory in po_add_gfa");
    }
    if (data) ::munmap(const_cast<char*>(data), size);
    ::close(fd);
    if (st != PO_OK) return st;
    return po_result_from_rows(h, rows.data(), rows.size(), rows_out);
}

po_status po_layout_edges(po_handle* h, po_result* rows, const po_layout_params* params, uint8_t* removed_reads_out,
                          po_result** edges_out) {
    if (!h || !rows || !params || !edges_out) return PO_ERR_INVALID;
    *edges_out = nullptr;
    if (rows->h != h) return fail(h, PO_ERR_INVALID, "po_layout_edges: the rows belong to another handle");
    if (rows->elem != sizeof(po_row)) return fail(h, PO_ERR_INVALID, "po_layout_edges needs a row result");
    if (params->reserved != 0 || !(params->max_overhang_rel == params->max_overhang_rel))
        return fail(h, PO_ERR_INVALID, "po_layout_edges: bad parameters");
    if (!ids_are_strand_pairs(h))
        return fail(h, PO_ERR_INVALID, "po_layout_edges needs reads added as name+\"+\" / name+\"-\" pairs");
    return new_edge_result(h, "po_layout_edges", edges_out,
                           [&](po_result* r) { return run_layout(h, rows, *params, removed_reads_out, r); });
}

po_status po_layout_reduce(po_handle* h, po_result* edges, const po_reduce_params* params, uint8_t* edge_flags_out,
                           po_result** kept_out) {
    if (!h || !edges || !params || !kept_out) return PO_ERR_INVALID;
    *kept_out = nullptr;
    return stage2_call(h, edges, "po_layout_reduce", params->reserved == 0 && params->length_fuzz >= 0, "a po_layout_edges result",
                       CANNOT_CLEAN_AGAIN, kept_out, [&](po_result* r) { return run_reduce(h, edges, *params, edge_flags_out, r); });
}

po_status po_layout_tips(po_handle* h, po_result* edges, const po_tips_params* params, uint8_t* edge_flags_out,
                         po_result** kept_out) {
    if (!h || !edges || !params || !kept_out) return PO_ERR_INVALID;
    *kept_out = nullptr;
    return stage2_call(h, edges, "po_layout_tips", params->reserved == 0,
                       "an edge result (po_layout_edges, po_layout_reduce, po_layout_tips)", CANNOT_CLEAN_AGAIN, kept_out,
                       [&](po_result* r) { return run_tips(h, edges, *params, edge_flags_out, r); });
}

po_status po_layout_diamonds(po_handle* h, po_result* edges, const po_diamond_params* params, uint8_t* edge_flags_out,
                             po_result** kept_out) {
    if (!h || !edges || !kept_out) return PO_ERR_INVALID;
    *kept_out = nullptr;
    return stage2_call(h, edges, "po_layout_diamonds", !params || params->reserved == 0,
                       "an edge result (po_layout_edges, po_layout_reduce, po_layout_tips, po_layout_diamonds)", CANNOT_CLEAN_AGAIN,
                       kept_out, [&](po_result* r) { return run_diamonds(h, edges, edge_flags_out, r); });
}

po_status po_layout_merge(po_handle* h, po_result* edges, const po_merge_params* params, uint8_t* edge_flags_out,
                          po_result** merged_out) {
    if (!h || !edges || !merged_out) return PO_ERR_INVALID;
    *merged_out = nullptr;
    return stage2_call(h, edges, "po_layout_merge", !params || params->reserved == 0,
                       "an edge result (po_layout_edges, po_layout_reduce, po_layout_tips, po_layout_diamonds)",
                       "the graph is merged already", merged_out, [&](po_result* r) { return run_merge(h, edges, edge_flags_out, r); });
}

po_status po_layout_coverage(po_handle* h, po_result* graph, po_result* rows, const po_coverage_params* params,
                             po_edge_coverage* coverage_out) {
    if (!h || !graph || !rows) return PO_ERR_INVALID;
    if (graph->h != h || rows->h != h) return fail(h, PO_ERR_INVALID, "po_layout_coverage: a result belongs to another handle");
    if (params && params->reserved != 0) return fail(h, PO_ERR_INVALID, "po_layout_coverage: bad parameters");
    // (no CPU fallback: without a usable GPU nothing below can be true of a result either)
    const po_status dev = init_device(h);
    if (dev != PO_OK) return dev;
    if (graph->elem != sizeof(po_edge) || !graph->kind_edges || graph->host_graph)
        return fail(h, PO_ERR_INVALID, "po_layout_coverage needs an edge result or a merged graph in the first position");
    if (rows->elem != sizeof(po_row) || rows->kind_edges) return fail(h, PO_ERR_INVALID, "po_layout_coverage needs a row result in the second position");
    if (graph->count && !coverage_out) return fail(h, PO_ERR_INVALID, "po_layout_coverage: no room for the coverage of the edges");
    return guarded_run(h, "po_layout_coverage", [&] { return run_coverage(h, graph, rows, coverage_out); });
}

po_status po_layout_components(po_handle* h, po_result* graph, const po_components_params* params, uint32_t* node_component_out,
                               uint32_t* edge_component_out, po_component* components_out, uint64_t* n_components_out) {
    return graph_call(h, graph, "po_layout_components", !params || params->reserved == 0, "components", n_components_out, [&] {
        return run_components(h, graph, node_component_out, edge_component_out, components_out, n_components_out);
    });
}

po_status po_layout_partition(po_handle* h, po_result* graph, const po_partition_params* params, uint32_t* node_scc_out,
                              uint8_t* node_flags_out, uint8_t* edge_class_out, po_scc* sccs_out, uint64_t* n_sccs_out) {
    return graph_call(h, graph, "po_layout_partition", !params || params->reserved == 0, "strongly connected components", n_sccs_out, [&] {
        return run_partition(h, graph, node_scc_out, node_flags_out, edge_class_out, sccs_out, n_sccs_out);
    });
}

po_status po_graph_from_edges(po_handle* h, const po_edge* edges, uint64_t n_edges, const uint32_t* node_order, uint64_t n_order,
                              po_result** out) {
    if (!h || !out || (!edges && n_edges) || (!node_order && n_order)) return PO_ERR_INVALID;
    *out = nullptr;
    if (n_edges >= 0x7FFFFF00ull) return fail(h, PO_ERR_CAPACITY, "po_graph_from_edges: too many edges for one call");
    const size_t n_ids = h->len.size();
    try {
        std::vector<uint8_t> in_order(n_ids, 0);
        for (uint64_t i = 0; i < n_order; ++i) {
            const uint32_t x = node_order[i];
            if (x >= n_ids) return fail(h, PO_ERR_INVALID, "po_graph_from_edges: the node order names a read the handle does not hold");
            if (in_order[x]) return fail(h, PO_ERR_INVALID, "po_graph_from_edges: a node appears twice in the node order");
            in_order[x] = 1;
        }
        std::vector<uint64_t> pairs(n_edges);
        for (uint64_t e = 0; e < n_edges; ++e) {
            const uint32_t u = edges[e].u, v = edges[e].v;
            if (u >= n_ids || v >= n_ids) return fail(h, PO_ERR_INVALID, "po_graph_from_edges: an edge names a read the handle does not hold");
            if (!in_order[u] || !in_order[v])
                return fail(h, PO_ERR_INVALID, "po_graph_from_edges: an edge has an end that is not in the node order");
            pairs[e] = ((uint64_t)u << 32) | v;
        }
        std::sort(pairs.begin(), pairs.end());
        if (std::adjacent_find(pairs.begin(), pairs.end()) != pairs.end())
            return fail(h, PO_ERR_INVALID, "po_graph_from_edges: an edge appears twice");
    } catch (const std::bad_alloc&) {
        return fail(h, PO_ERR_NOMEM, "out of host memory in po_graph_from_edges");
    }
    // (no CPU fallback: the node order of a graph result lives on the device)
    PO_TRY(init_device(h));
    return new_edge_result(h, "po_graph_from_edges", out, [&](po_result* r) {
        r->elem = sizeof(po_edge);
        r->kind_edges = true;
        r->host_graph = true;
        // rank words: the place in the node order, all ones for every other read (and behind the reads)
        const size_t nrank_bytes = std::max<size_t>(n_ids * 8, 256);
        PO_TRY(ensure_nrank(h, r, nrank_bytes));
        PO_TRY(ensure_host(h, h->scratch_host, nrank_bytes));
        std::memset(h->scratch_host.p, 0xFF, nrank_bytes);
        uint64_t* words = static_cast<uint64_t*>(h->scratch_host.p);
        for (uint64_t i = 0; i < n_order; ++i) words[node_order[i]] = i;
        HIP_TRY(h, hipMemcpyAsync(r->d_nrank.p, words, nrank_bytes, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (n_edges) {
            void* copy = std::malloc(n_edges * sizeof(po_edge));
            if (!copy) return fail(h, PO_ERR_NOMEM, "out of host memory for the edge array");
            std::memcpy(copy, edges, n_edges * sizeof(po_edge));
            r->host = copy;
            r->host_malloced = true;
        }
        r->count = n_edges;
        return PO_OK;
    });
}

po_status po_get_layout_stats(const po_handle* h, po_layout_stats* out) { return get_stats(h, &po_handle::lstats, out); }
po_status po_get_node_order_stats(const po_handle* h, po_node_order_stats* out) { return get_stats(h, &po_handle::nostats, out); }
po_status po_get_reduce_stats(const po_handle* h, po_reduce_stats* out) { return get_stats(h, &po_handle::rstats, out); }
po_status po_get_tips_stats(const po_handle* h, po_tips_stats* out) { return get_stats(h, &po_handle::tstats, out); }
po_status po_get_diamond_stats(const po_handle* h, po_diamond_stats* out) { return get_stats(h, &po_handle::dstats, out); }
po_status po_get_merge_stats(const po_handle* h, po_merge_stats* out) { return get_stats(h, &po_handle::mstats, out); }
po_status po_get_coverage_stats(const po_handle* h, po_coverage_stats* out) { return get_stats(h, &po_handle::cstats, out); }
po_status po_get_components_stats(const po_handle* h, po_components_stats* out) { return get_stats(h, &po_handle::ccstats, out); }
po_status po_get_partition_stats(const po_handle* h, po_partition_stats* out) { return get_stats(h, &po_handle::pstats, out); }

po_status po_layout_superbubbles(po_handle* h, po_result* graph, const po_superbubble_params* params, uint32_t* node_exit_out,
                                 uint32_t* node_inside_out, uint8_t* node_flags_out, po_superbubble* bubbles_out, uint64_t* n_bubbles_out) {
    return graph_call(h, graph, "po_layout_superbubbles", !params || params->reserved == 0, "superbubbles", n_bubbles_out, [&] {
        return run_superbubbles(h, graph, node_exit_out, node_inside_out, node_flags_out, bubbles_out, n_bubbles_out);
    });
}

po_status po_get_superbubble_stats(const po_handle* h, po_superbubble_stats* out) { return get_stats(h, &po_handle::sbstats, out); }

po_status po_layout_superbubbles_all(po_handle* h, po_result* graph, const po_superbubble_all_params* params, uint32_t* node_exit_out,
                                     uint32_t* node_inside_out, uint8_t* node_flags_out, po_superbubble* bubbles_out, uint64_t* n_bubbles_out) {
    return graph_call(h, graph, "po_layout_superbubbles_all", !params || params->reserved == 0, "superbubbles", n_bubbles_out, [&] {
        return run_superbubbles_all(h, graph, node_exit_out, node_inside_out, node_flags_out, bubbles_out, n_bubbles_out);
    });
}

po_status po_get_superbubble_all_stats(const po_handle* h, po_superbubble_all_stats* out) { return get_stats(h, &po_handle::sastats, out); }

po_status po_layout_bubblechains(po_handle* h, po_result* graph, const po_bubblechain_params* params, uint32_t* node_chain_out,
                                 uint32_t* node_bubble_out, uint32_t* edge_chain_out, po_bubblechain* chains_out, uint64_t* n_chains_out) {
    return graph_call(h, graph, "po_layout_bubblechains", !params || (params->reserved == 0 && params->min_nodes != 0), "bubble chains",
                      n_chains_out, [&] {
        return run_bubblechains(h, graph, params ? params->min_nodes : 1u, node_chain_out, node_bubble_out, edge_chain_out, chains_out,
                                n_chains_out);
    });
}

po_status po_get_bubblechain_stats(const po_handle* h, po_bubblechain_stats* out) { return get_stats(h, &po_handle::bcstats, out); }

po_status po_layout_bubblechains_all(po_handle* h, po_result* graph, const po_bubblechain_params* params, uint32_t* node_chain_out,
                                     uint32_t* node_bubble_out, uint32_t* edge_chain_out, po_bubblechain* chains_out, uint64_t* n_chains_out) {
    return graph_call(h, graph, "po_layout_bubblechains_all", !params || (params->reserved == 0 && params->min_nodes != 0), "bubble chains",
                      n_chains_out, [&] {
        return run_bubblechains_all(h, graph, params ? params->min_nodes : 1u, node_chain_out, node_bubble_out, edge_chain_out, chains_out,
                                    n_chains_out);
    });
}

po_status po_get_bubblechain_all_stats(const po_handle* h, po_bubblechain_all_stats* out) { return get_stats(h, &po_handle::bcastats, out); }

po_status po_layout_contigs_all(po_handle* h, po_result* graph, const po_contig_params* params, const uint8_t* exclude_in,
                                uint32_t* edge_contig_out, uint32_t* edge_pos_out, po_contig* contigs_out, uint64_t* n_contigs_out) {
    return graph_call(h, graph, "po_layout_contigs_all", !params || (params->reserved == 0 && params->min_nodes != 0), "contigs", n_contigs_out,
                      [&] {
        return run_contigs(h, graph, params ? params->min_contig_len : 5000ull, params ? params->min_nodes : 1u, exclude_in, edge_contig_out,
                           edge_pos_out, contigs_out, n_contigs_out, true);
    });
}

po_status po_layout_contigs(po_handle* h, po_result* graph, const po_contig_params* params, const uint8_t* exclude_in,
                            uint32_t* edge_contig_out, uint32_t* edge_pos_out, po_contig* contigs_out, uint64_t* n_contigs_out) {
    return graph_call(h, graph, "po_layout_contigs", !params || (params->reserved == 0 && params->min_nodes != 0), "contigs", n_contigs_out, [&] {
        return run_contigs(h, graph, params ? params->min_contig_len : 5000ull, params ? params->min_nodes : 1u, exclude_in, edge_contig_out,
                           edge_pos_out, contigs_out, n_contigs_out);
    });
}

po_status po_get_contig_stats(const po_handle* h, po_contig_stats* out) { return get_stats(h, &po_handle::ctstats, out); }

po_status po_phase_branch(po_handle* h, const po_phase_params* params, const po_phase_input* input, uint32_t* cand_out, uint32_t* ext_out,
                          double* rl_out, uint64_t cap, double* table_out, uint64_t* n_out) {
    if (!h) return PO_ERR_INVALID;
    if (!n_out) return fail(h, PO_ERR_INVALID, "po_phase_branch: no room for the number of entries");
    *n_out = 0;
    if (!params || !input) return fail(h, PO_ERR_INVALID, "po_phase_branch: no parameters");
    uint64_t Pk = 0;
    const std::string said = phase_check(*params, *input, Pk);
    if (!said.empty()) return fail(h, PO_ERR_INVALID, said);
    // (no CPU fallback)
    PO_TRY(init_device(h));
    return guarded_run(h, "po_phase_branch", [&] {
        return run_phase(h, *params, *input, (uint32_t)Pk, cand_out, ext_out, rl_out, cap, table_out, n_out);
    });
}

po_status po_get_phase_stats(const po_handle* h, po_phase_stats* out) { return get_stats(h, &po_handle::phstats, out); }

po_status po_walk_create(po_handle* h, uint32_t ploidy, po_result** walk_out) {
    if (!h) return PO_ERR_INVALID;
    if (!walk_out) return fail(h, PO_ERR_INVALID, "po_walk_create: no room for the walk");
    *walk_out = nullptr;
    if (ploidy < 1 || ploidy > po::PH_MAX_K) return fail(h, PO_ERR_INVALID, "po_walk_create: the ploidy must be 1 to 8");
    // (the device is not touched: a walk that has not advanced holds nothing there)
    return new_edge_result(h, "po_walk_create", walk_out, [&](po_result* r) {
        r->special = WALK_KIND;
        r->elem = 1;
        r->wk_k = ploidy;
        walk_clear(r);
        return PO_OK;
    });
}

po_status po_walk_reset(po_result* walk) {
    if (!walk) return PO_ERR_INVALID;
    if (walk->special != WALK_KIND) return fail(walk->h, PO_ERR_INVALID, "po_walk_reset needs the result of po_walk_create");
    walk_clear(walk);
    return PO_OK;
}

po_status po_walk_info_get(const po_result* walk, po_walk_info* info) {
    if (!walk || !info) return PO_ERR_INVALID;
    if (walk->special != WALK_KIND) return fail(walk->h, PO_ERR_INVALID, "po_walk_info_get needs the result of po_walk_create");
    info->ploidy = walk->wk_k;
    info->n_cands = walk->wk_n_cands;
    info->depth = walk_depth(walk);
    info->start_of_block = info->depth == 0;
    info->n_block_reads = walk->wk_route == 2 ? walk->rs_n_block : walk->wk_reads.size();
    return PO_OK;
}

po_status po_walk_step(po_handle* h, po_result* walk, const po_phase_params* params, const po_phase_input* input, const uint32_t* b_reads,
                       uint32_t advance, uint32_t* cand_out, uint32_t* ext_out, double* rl_out, uint64_t cap, uint64_t* n_out) {
    if (!h) return PO_ERR_INVALID;
    if (!n_out) return fail(h, PO_ERR_INVALID, "po_walk_step: no room for the number of entries");
    *n_out = 0;
    if (!walk) return fail(h, PO_ERR_INVALID, "po_walk_step: no walk");
    if (!params || !input) return fail(h, PO_ERR_INVALID, "po_walk_step: no parameters");
    std::string said = walk_check(h, walk, *params, *input, b_reads);
    if (!said.empty()) return fail(h, PO_ERR_INVALID, said);
    uint64_t Pk = 0;
    {
        // (po_phase_branch's own checks, on the bubble with every read set empty)
        std::vector<uint32_t> no_sets((size_t)params->n_cands * params->ploidy + 1, 0u);
        po_phase_input as_branch = *input;
        as_branch.set_off = no_sets.data();
        said = phase_check(*params, as_branch, Pk, "po_walk_step");
    }
    if (!said.empty()) return fail(h, PO_ERR_INVALID, said);
    // (no CPU fallback)
    PO_TRY(init_device(h));
    return guarded_run(h, "po_walk_step", [&] {
        return run_walk_step(h, walk, *params, *input, b_reads, advance != 0, cand_out, ext_out, rl_out, cap, n_out);
    });
}

po_status po_walk_relevant(po_handle* h, po_result* walk, po_result* index, const po_walk_relevant_params* params,
                           const po_relevant_input* input, po_result** out) {
    if (!h) return PO_ERR_INVALID;
    const std::string name = "po_walk_relevant: ";
    if (!out) return fail(h, PO_ERR_INVALID, name + "no room for the result");
    *out = nullptr;
    if (!walk) return fail(h, PO_ERR_INVALID, name + "no walk");
    if (!index) return fail(h, PO_ERR_INVALID, name + "no index");
    if (!params || !input) return fail(h, PO_ERR_INVALID, name + "no parameters");
    if (params->reserved) return fail(h, PO_ERR_INVALID, name + "bad parameters");
    if (input->prev_graph || input->n_prev_graph || input->prev_aligning || input->n_prev_aligning)
        return fail(h, PO_ERR_INVALID, name + "prev_graph and prev_aligning must be NULL with count 0: the two sets are the walk's");
    if (walk->special != WALK_KIND) return fail(h, PO_ERR_INVALID, name + "needs the result of po_walk_create");
    if (walk->h != h) return fail(h, PO_ERR_INVALID, name + "the walk belongs to another handle");
    const po_relevant_params as_gather{params->mode, params->min_spanning_reads, 0, 0};
    const std::string said = relevant_check(h, index, &as_gather, input, "po_walk_relevant");
    if (!said.empty()) return fail(h, PO_ERR_INVALID, said);
    if (walk->wk_route == 1)
        return fail(h, PO_ERR_INVALID, name + "the block advanced by po_walk_step: the two routes do not mix before po_walk_reset");
    // (no CPU fallback)
    PO_TRY(init_device(h));
    return new_edge_result(h, "po_walk_relevant", out, [&](po_result* r) {
        return run_relevant(h, index, as_gather, *input, r, walk, params->without_prev_graph != 0);
    });
}

po_status po_walk_step_resident(po_handle* h, po_result* walk, po_result* rel, const po_phase_params* params, const po_phase_input* input,
                                uint32_t advance, uint32_t* cand_out, uint32_t* ext_out, double* rl_out, uint64_t cap, uint64_t* n_out) {
    if (!h) return PO_ERR_INVALID;
    const std::string name = "po_walk_step_resident: ";
    if (!n_out) return fail(h, PO_ERR_INVALID, name + "no room for the number of entries");
    *n_out = 0;
    if (!walk) return fail(h, PO_ERR_INVALID, name + "no walk");
    if (!rel) return fail(h, PO_ERR_INVALID, name + "no gather");
    if (!params || !input) return fail(h, PO_ERR_INVALID, name + "no parameters");
    uint64_t Pk = 0;
    const std::string said = resident_check(h, walk, rel, *params, *input, Pk);
    if (!said.empty()) return fail(h, PO_ERR_INVALID, said);
    // (no CPU fallback)
    PO_TRY(init_device(h));
    return guarded_run(h, "po_walk_step_resident", [&] {
        return run_walk_step_resident(h, walk, rel, *params, *input, advance != 0, cand_out, ext_out, rl_out, cap, n_out);
    });
}

po_status po_walk_prev_copy(po_result* walk, uint32_t which, uint32_t* ids_out, uint64_t cap, uint64_t* n_out) {
    if (!walk) return PO_ERR_INVALID;
    po_handle* h = walk->h;
    if (!n_out) return fail(h, PO_ERR_INVALID, "po_walk_prev_copy: no room for the number of ids");
    *n_out = 0;
    if (walk->special != WALK_KIND) return fail(h, PO_ERR_INVALID, "po_walk_prev_copy needs the result of po_walk_create");
    if (which > 1) return fail(h, PO_ERR_INVALID, "po_walk_prev_copy: which must be 0 (prev_graph) or 1 (prev_aligning)");
    if (!walk->d_rs_prev.p || walk->rs_clear_prev) return PO_OK;   // (both sets are empty: nothing lies on the device)
    PO_TRY(init_device(h));
    return guarded_run(h, "po_walk_prev_copy", [&] { return run_walk_prev_copy(h, walk, which, ids_out, cap, n_out); });
}

po_status po_walk_best(po_result* walk, uint32_t* cands_out, uint64_t cap, uint64_t* n_out, double* max_rl_out) {
    if (!walk) return PO_ERR_INVALID;
    po_handle* h = walk->h;
    if (!n_out) return fail(h, PO_ERR_INVALID, "po_walk_best: no room for the number of candidates");
    *n_out = 0;
    const std::string said = walk_asked(walk, "po_walk_best", nullptr, 0);
    if (!said.empty()) return fail(h, PO_ERR_INVALID, said);
    if (walk_depth(walk)) PO_TRY(init_device(h));
    return guarded_run(h, "po_walk_best", [&] { return run_walk_best(h, walk, cands_out, cap, n_out, max_rl_out); });
}

po_status po_walk_history(po_result* walk, const uint32_t* cands, uint64_t n, uint32_t* ext_out) {
    if (!walk) return PO_ERR_INVALID;
    po_handle* h = walk->h;
    const std::string said = walk_asked(walk, "po_walk_history", cands, n);
    if (!said.empty()) return fail(h, PO_ERR_INVALID, said);
    if (n && walk_depth(walk) && !ext_out) return fail(h, PO_ERR_INVALID, "po_walk_history: no room for the extensions");
    if (walk_depth(walk)) PO_TRY(init_device(h));
    return guarded_run(h, "po_walk_history", [&] { return run_walk_history(h, walk, cands, (uint32_t)n, ext_out); });
}

po_status po_walk_read_sets(po_result* walk, const uint32_t* cands, uint64_t n, uint64_t* off_out, uint32_t* ids_out, uint64_t cap,
                            uint64_t* n_ids_out) {
    if (!walk) return PO_ERR_INVALID;
    po_handle* h = walk->h;
    if (!n_ids_out) return fail(h, PO_ERR_INVALID, "po_walk_read_sets: no room for the number of ids");
    *n_ids_out = 0;
    const std::string said = walk_asked(walk, "po_walk_read_sets", cands, n);
    if (!said.empty()) return fail(h, PO_ERR_INVALID, said);
    if (walk_depth(walk)) PO_TRY(init_device(h));
    return guarded_run(h, "po_walk_read_sets", [&] { return run_walk_read_sets(h, walk, cands, (uint32_t)n, off_out, ids_out, cap, n_ids_out); });
}

po_status po_get_walk_stats(const po_handle* h, po_walk_stats* out) { return get_stats(h, &po_handle::wkstats, out); }

po_status po_phase_index(po_handle* h, po_result* rows, po_result** index_out) {
    if (!h || !rows || !index_out) return PO_ERR_INVALID;
    *index_out = nullptr;
    if (rows->h != h) return fail(h, PO_ERR_INVALID, "po_phase_index: the rows belong to another handle");
    if (rows->elem != sizeof(po_row) || rows->kind_edges || rows->special) return fail(h, PO_ERR_INVALID, "po_phase_index needs a row result");
    if (2 * rows->count >= (1ull << 31)) return fail(h, PO_ERR_CAPACITY, "po_phase_index: more than 2^30 - 1 rows in one call");
    // (no CPU fallback)
    PO_TRY(init_device(h));
    return new_edge_result(h, "po_phase_index", index_out, [&](po_result* r) { return run_phase_index(h, rows, r); });
}

po_status po_phase_index_copy(po_result* index, uint64_t* off_out, po_alignment* entries_out, uint64_t cap, uint64_t* n_out) {
    if (!index) return PO_ERR_INVALID;
    po_handle* h = index->h;
    if (!n_out) return fail(h, PO_ERR_INVALID, "po_phase_index_copy: no room for the number of entries");
    *n_out = 0;
    if (index->special != 1) return fail(h, PO_ERR_INVALID, "po_phase_index_copy needs the result of po_phase_index");
    static_assert(sizeof(po_alignment) == sizeof(po::RrEntry), "an entry of the index is a po_alignment");
    const size_t n_off = (size_t)index->ix_n_ids + 1, n_give = (size_t)std::min<uint64_t>(cap, index->ix_n_keys);
    return guarded_run(h, "po_phase_index_copy", [&] {
        if (off_out) {
            std::vector<uint32_t> off(n_off);
            HIP_TRY(h, hipMemcpyAsync(off.data(), index->d_ixoff.p, n_off * 4, hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(h, hipStreamSynchronize(h->stream));
            for (size_t i = 0; i < n_off; ++i) off_out[i] = off[i];
        }
        if (entries_out && n_give) {
            HIP_TRY(h, hipMemcpyAsync(entries_out, index->d_ixent.p, n_give * sizeof(po_alignment), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(h, hipStreamSynchronize(h->stream));
        }
        *n_out = index->ix_n_keys;
        return PO_OK;
    });
}

po_status po_get_phase_index_stats(const po_handle* h, po_phase_index_stats* out) { return get_stats(h, &po_handle::pxstats, out); }

po_status po_phase_relevant(po_handle* h, po_result* index, const po_relevant_params* params, const po_relevant_input* input,
                            po_result** out) {
    if (!h) return PO_ERR_INVALID;
    if (!out) return fail(h, PO_ERR_INVALID, "po_phase_relevant: no room for the result");
    *out = nullptr;
    if (!index) return fail(h, PO_ERR_INVALID, "po_phase_relevant: no index");
    const std::string said = relevant_check(h, index, params, input);
    if (!said.empty()) return fail(h, PO_ERR_INVALID, said);
    // (no CPU fallback)
    PO_TRY(init_device(h));
    return new_edge_result(h, "po_phase_relevant", out, [&](po_result* r) { return run_relevant(h, index, *params, *input, r); });
}

po_status po_relevant_sizes(const po_result* out, po_relevant_dims* sizes) {
    if (!out || !sizes) return PO_ERR_INVALID;
    if (out->special != 2) return fail(out->h, PO_ERR_INVALID, "po_relevant_sizes needs the result of po_phase_relevant");
    *sizes = out->rv;
    return PO_OK;
}

po_status po_relevant_copy(po_result* out, uint32_t* cur_aligning, uint32_t* rel_reads, int32_t* overlap_max, uint32_t* aln_off,
                           uint32_t* aln_b, int32_t* aln_a0, int32_t* aln_a1, uint32_t* b_reads) {
    if (!out) return PO_ERR_INVALID;
    if (out->special != 2) return fail(out->h, PO_ERR_INVALID, "po_relevant_copy needs the result of po_phase_relevant");
    if (out->rv_resident) {
        // a gather of po_walk_relevant: the arrays are fetched from the walk's buffers, where the gather left them
        po_handle* h = out->h;
        const std::string said = gather_live(nullptr, out, "po_relevant_copy");
        if (!said.empty()) return fail(h, PO_ERR_INVALID, said);
        if (out->rv_empty) {
            if (aln_off) aln_off[0] = 0;
            return PO_OK;
        }
        PO_TRY(init_device(h));
        const DevBuf* B = out->rv_walk->d_rs_rel;
        const size_t n_ca = out->rv.n_cur_aligning, n_rel = out->rv.n_relevant, n_aln = out->rv.n_alignments, n_b = out->rv.n_b;
        return guarded_run(h, "po_relevant_copy", [&] {
            return land_outputs(h, {{B[XB_CA].p, n_ca * 4, cur_aligning}, {B[XB_REL].p, n_rel * 4, rel_reads}, {B[XB_OM].p, n_rel * 4, overlap_max},
                                    {B[XB_ALNOFF].p, (n_rel + 1) * 4, aln_off}, {B[XB_ALNB].p, n_aln * 4, aln_b}, {B[XB_A0].p, n_aln * 4, aln_a0},
                                    {B[XB_A1].p, n_aln * 4, aln_a1}, {B[XB_B].p, n_b * 4, b_reads}}, B[XB_CNT].as<unsigned long long>(), 1);
        });
    }
    auto give = [](void* dst, const void* src, size_t n) {
        if (dst && n) std::memcpy(dst, src, n * 4);
    };
    give(cur_aligning, out->rv_ca.data(), out->rv_ca.size());
    give(rel_reads, out->rv_rel.data(), out->rv_rel.size());
    give(overlap_max, out->rv_om.data(), out->rv_om.size());
    if (aln_off && out->rv_alnoff.empty()) aln_off[0] = 0;   // (an empty cur_graph: one offset, 0)
    give(aln_off, out->rv_alnoff.data(), out->rv_alnoff.size());
    give(aln_b, out->rv_alnb.data(), out->rv_alnb.size());
    give(aln_a0, out->rv_a0.data(), out->rv_a0.size());
    give(aln_a1, out->rv_a1.data(), out->rv_a1.size());
    give(b_reads, out->rv_b.data(), out->rv_b.size());
    return PO_OK;
}

po_status po_get_relevant_stats(const po_handle* h, po_relevant_stats* out) { return get_stats(h, &po_handle::rvstats, out); }

po_status po_spell(po_handle* h, const po_spell_input* in, po_result** out) {
    if (!h) return PO_ERR_INVALID;
    if (!out) return fail(h, PO_ERR_INVALID, "po_spell: no room for the result");
    *out = nullptr;
    if (!in) return fail(h, PO_ERR_INVALID, "po_spell: no input");
    if (in->n_pieces >= 0xFFFFFFFFull || in->n_seqs >= 0xFFFFFFFFull)
        return fail(h, PO_ERR_CAPACITY, "po_spell: more than 2^32 - 2 pieces or sequences in one call");
    uint64_t n_bytes = 0, n_patched = 0;
    const std::string said = spell_check(h, *in, &n_bytes, &n_patched);
    if (!said.empty()) return fail(h, PO_ERR_INVALID, said);
    // (decided from the host's sum, before anything is allocated: the caller splits the call)
    if (n_bytes > SPELL_MAX_BYTES)
        return fail(h, PO_ERR_CAPACITY, "po_spell: " + std::to_string(n_bytes) + " bytes in one call, at most 2^32 - 16");
    // (no CPU fallback)
    PO_TRY(init_device(h));
    return new_edge_result(h, "po_spell", out, [&](po_result* r) { return run_spell(h, *in, n_bytes, n_patched, r); });
}

po_status po_spell_sizes(const po_result* out, uint64_t* n_seqs, uint64_t* n_bytes) {
    if (!out || !n_seqs || !n_bytes) return PO_ERR_INVALID;
    if (out->special != 3) return fail(out->h, PO_ERR_INVALID, "po_spell_sizes needs the result of po_spell");
    *n_seqs = out->sp_off.size() - 1;
    *n_bytes = out->sp_off.back();
    return PO_OK;
}

po_status po_spell_copy(po_result* out, uint64_t* seq_byte_off, uint8_t* bytes, uint64_t cap) {
    if (!out) return PO_ERR_INVALID;
    po_handle* h = out->h;
    if (out->special != 3) return fail(h, PO_ERR_INVALID, "po_spell_copy needs the result of po_spell");
    if (seq_byte_off) std::memcpy(seq_byte_off, out->sp_off.data(), out->sp_off.size() * 8);
    const uint64_t n_give = bytes ? std::min<uint64_t>(cap, out->sp_off.back()) : 0;
    if (!n_give) return PO_OK;
    // through the page-locked landing zone, 64 MB at a time
    constexpr uint64_t STEP = 64ull << 20;
    return guarded_run(h, "po_spell_copy", [&] {
        PO_TRY(ensure_host(h, h->scratch_host, (size_t)std::min(n_give, STEP)));
        for (uint64_t at = 0; at < n_give; at += STEP) {
            const size_t k = (size_t)std::min(STEP, n_give - at);
            HIP_TRY(h, hipMemcpyAsync(h->scratch_host.p, out->d_rows.as<char>() + at, k, hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(h, hipStreamSynchronize(h->stream));
            std::memcpy(bytes + at, h->scratch_host.p, k);
        }
        return PO_OK;
    });
}

po_status po_get_spell_stats(const po_handle* h, po_spell_stats* out) { return get_stats(h, &po_handle::spstats, out); }

po_status po_phase_paths(po_handle* h, po_result* graph, const po_paths_params* params, po_result** out) {
    const char* const name = "po_phase_paths";
    if (!h) return PO_ERR_INVALID;
    if (!out) return fail(h, PO_ERR_INVALID, std::string(name) + ": no room for the result");
    *out = nullptr;
    if (!graph) return fail(h, PO_ERR_INVALID, std::string(name) + ": no graph");
    if (graph->h != h) return fail(h, PO_ERR_INVALID, std::string(name) + ": the graph belongs to another handle");
    if (params && params->reserved != 0) return fail(h, PO_ERR_INVALID, std::string(name) + ": bad parameters");
    if (graph->elem != sizeof(po_edge) || !graph->kind_edges)
        return fail(h, PO_ERR_INVALID, std::string(name) + " needs an edge result, a merged graph or a po_graph_from_edges result");
    // (no CPU fallback)
    PO_TRY(init_device(h));
    return new_edge_result(h, name, out, [&](po_result* r) { return run_paths(h, graph, params ? params->max_paths : 0, r); });
}

po_status po_paths_sizes(const po_result* out, po_paths_dims* dims) {
    if (!out || !dims) return PO_ERR_INVALID;
    if (out->special != 4) return fail(out->h, PO_ERR_INVALID, "po_paths_sizes needs the result of po_phase_paths");
    *dims = out->pp;
    return PO_OK;
}

po_status po_paths_copy(po_result* out, po_bubble_paths* bubbles, uint64_t* inside_off, uint32_t* inside_nodes, uint64_t* pred_off,
                        uint32_t* pred_node, int32_t* pred_weight, uint64_t* bubble_path_off, uint64_t* path_off, uint32_t* path_nodes) {
    if (!out) return PO_ERR_INVALID;
    po_handle* h = out->h;
    if (out->special != 4) return fail(h, PO_ERR_INVALID, "po_paths_copy needs the result of po_phase_paths");
    const po_paths_dims& D = out->pp;
    if (!D.n_bubbles) {   // (nothing on the device: one offset each, 0)
        for (uint64_t* p : {inside_off, pred_off, bubble_path_off, path_off})
            if (p) p[0] = 0;
        return PO_OK;
    }
    return guarded_run(h, "po_paths_copy", [&] {
        hipStream_t st = h->stream;
        // straight into the caller's arrays; the device holds the offsets in 32 bits: they are widened from a staging copy
        auto give = [&](void* dst, int k, size_t bytes) -> po_status {
            if (dst && bytes) HIP_TRY(h, hipMemcpyAsync(dst, out->d_pp[k].p, bytes, hipMemcpyDeviceToHost, st));
            return PO_OK;
        };
        const size_t nb1 = (size_t)D.n_bubbles + 1, np1 = (size_t)D.n_listed_paths + 1;
        std::vector<uint32_t> stage[4];
        const struct { uint64_t* dst; int k; size_t n; } offs[4] = {{inside_off, PR_INOFF, nb1}, {pred_off, PR_PREDOFF, nb1},
                                                                    {bubble_path_off, PR_BPO, nb1}, {path_off, PR_POFF, np1}};
        for (int i = 0; i < 4; ++i)
            if (offs[i].dst) {
                stage[i].resize(offs[i].n);
                PO_TRY(give(stage[i].data(), offs[i].k, offs[i].n * 4));
            }
        PO_TRY(give(bubbles, PR_TABLE, (size_t)D.n_bubbles * sizeof(po_bubble_paths)));
        PO_TRY(give(inside_nodes, PR_INNODES, (size_t)D.n_inside_nodes * 4));
        PO_TRY(give(pred_node, PR_PREDNODE, (size_t)D.n_preds * 4));
        PO_TRY(give(pred_weight, PR_PREDW, (size_t)D.n_preds * 4));
        PO_TRY(give(path_nodes, PR_PATHS, (size_t)D.n_path_nodes * 4));
        HIP_TRY(h, hipStreamSynchronize(st));
        for (int i = 0; i < 4; ++i)
            if (offs[i].dst)
                for (size_t j = 0; j < offs[i].n; ++j) offs[i].dst[j] = stage[i][j];
        return PO_OK;
    });
}

po_status po_get_paths_stats(const po_handle* h, po_paths_stats* out) { return get_stats(h, &po_handle::ppstats, out); }

po_status po_phase_large(po_handle* h, po_result* paths, const po_large_params* params, const po_large_input* input, uint64_t* best_out,
                         double* best_score_out, double* scores_out, uint32_t* n_best_out) {
    const std::string name = "po_phase_large: ";
    if (!h) return PO_ERR_INVALID;
    if (!n_best_out) return fail(h, PO_ERR_INVALID, name + "no room for the number of best paths");
    *n_best_out = 0;
    if (!paths) return fail(h, PO_ERR_INVALID, name + "no paths result");
    if (!params || !input) return fail(h, PO_ERR_INVALID, name + "no parameters");
    if (!best_out || !best_score_out) return fail(h, PO_ERR_INVALID, name + "no room for the best paths");
    const std::string said = large_check(*params, *input);
    if (!said.empty()) return fail(h, PO_ERR_INVALID, said);
    if (paths->special != 4) return fail(h, PO_ERR_INVALID, "po_phase_large needs the result of po_phase_paths");
    if (paths->h != h) return fail(h, PO_ERR_INVALID, name + "the paths result belongs to another handle");
    if (params->bubble >= paths->pp.n_bubbles)
        return fail(h, PO_ERR_INVALID, name + "bubble " + std::to_string(params->bubble) + " is not below the " +
                                           std::to_string(paths->pp.n_bubbles) + " bubbles of the result");
    // (no CPU fallback)
    PO_TRY(init_device(h));
    return guarded_run(h, "po_phase_large", [&] { return run_large(h, paths, *params, *input, best_out, best_score_out, scores_out, n_best_out); });
}

po_status po_get_large_stats(const po_handle* h, po_large_stats* out) { return get_stats(h, &po_handle::lgstats, out); }

po_status po_paths_copy_paths(po_result* paths, uint64_t first, uint64_t count, uint64_t* path_off_out, uint32_t* path_nodes_out, uint64_t cap,
                              uint64_t* n_nodes_out) {
    if (!paths) return PO_ERR_INVALID;
    po_handle* h = paths->h;
    const std::string name = "po_paths_copy_paths: ";
    if (!n_nodes_out) return fail(h, PO_ERR_INVALID, name + "no room for the number of nodes");
    *n_nodes_out = 0;
    if (paths->special != 4) return fail(h, PO_ERR_INVALID, "po_paths_copy_paths needs the result of po_phase_paths");
    const uint64_t n_listed = paths->pp.n_listed_paths;
    if (first > n_listed || count > n_listed - first)
        return fail(h, PO_ERR_INVALID, name + "paths " + std::to_string(first) + " .. " + std::to_string(first) + " + " + std::to_string(count) +
                                           " end past the " + std::to_string(n_listed) + " listed paths");
    if (!count) {
        if (path_off_out) path_off_out[0] = 0;
        return PO_OK;
    }
    return guarded_run(h, "po_paths_copy_paths", [&] {
        hipStream_t st = h->stream;
        std::vector<uint32_t> off((size_t)count + 1);
        HIP_TRY(h, hipMemcpyAsync(off.data(), paths->d_pp[PR_POFF].as<uint32_t>() + first, ((size_t)count + 1) * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipStreamSynchronize(st));
        const uint64_t lo = off[0], hi = off[(size_t)count];
        if (hi < lo || hi > paths->pp.n_path_nodes) return fail(h, PO_ERR_HIP, "internal: the path offsets of po_paths_copy_paths do not add up");
        *n_nodes_out = hi - lo;
        if (path_nodes_out && cap < hi - lo)
            return fail(h, PO_ERR_CAPACITY, name + "the paths hold " + std::to_string(hi - lo) + " nodes, there is room for " + std::to_string(cap));
        if (path_nodes_out && hi > lo) {
            HIP_TRY(h, hipMemcpyAsync(path_nodes_out, paths->d_pp[PR_PATHS].as<uint32_t>() + lo, (size_t)(hi - lo) * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(h, hipStreamSynchronize(st));
        }
        if (path_off_out)
            for (size_t j = 0; j <= (size_t)count; ++j) path_off_out[j] = off[j] - lo;
        return PO_OK;
    });
}

po_status po_result_merged_paths(po_result* r, uint64_t* n_paths, uint64_t* n_members, uint64_t* offsets_out, uint64_t cap_paths,
                                 uint32_t* members_out, int32_t* prefix_out, uint64_t cap_members, int64_t* lengths_out) {
    if (!r || !n_paths || !n_members) return PO_ERR_INVALID;
    *n_paths = *n_members = 0;
    po_handle* h = r->h;
    if (!h) return PO_ERR_INVALID;
    if (!r->merged) return fail(h, PO_ERR_INVALID, "po_result_merged_paths needs a po_layout_merge result");
    const uint64_t K = r->n_merged, m = r->n_members;
    *n_paths = K;
    *n_members = m;
    try {
        (void)hipSetDevice(h->device);
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (offsets_out && cap_paths >= K) {
            std::vector<uint32_t> off(K);
            if (K) HIP_TRY(h, hipMemcpy(off.data(), r->d_moff.p, K * 4, hipMemcpyDeviceToHost));
            for (uint64_t k = 0; k < K; ++k) offsets_out[k] = off[k];
            offsets_out[K] = m;
        }
        if (lengths_out && cap_paths >= K && K) HIP_TRY(h, hipMemcpy(lengths_out, r->d_mlen.p, K * 8, hipMemcpyDeviceToHost));
        if (members_out && cap_members >= m && m) HIP_TRY(h, hipMemcpy(members_out, r->d_member.p, m * 4, hipMemcpyDeviceToHost));
        if (prefix_out && cap_members >= m && m) HIP_TRY(h, hipMemcpy(prefix_out, r->d_prefix.p, m * 4, hipMemcpyDeviceToHost));
    } catch (const std::bad_alloc&) {
        return fail(h, PO_ERR_NOMEM, "out of host memory in po_result_merged_paths");
    }
    return PO_OK;
}

po_status po_result_node_order(po_result* r, uint32_t* nodes_out, uint64_t cap, uint64_t* n_out) {
    if (!r || !n_out || (!nodes_out && cap)) return PO_ERR_INVALID;
    *n_out = 0;
    po_handle* h = r->h;
    if (!h) return PO_ERR_INVALID;
    if (!r->kind_edges || !r->d_nrank.p) return fail(h, PO_ERR_INVALID, "po_result_node_order needs an edge result");
    const size_t n_nodes = h->len.size() + (r->merged ? (size_t)r->n_merged : 0);   // (merged node k is node reads + k)
    try {
        std::vector<unsigned long long> rank(n_nodes);
        (void)hipSetDevice(h->device);
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (n_nodes) HIP_TRY(h, hipMemcpy(rank.data(), r->d_nrank.p, n_nodes * 8, hipMemcpyDeviceToHost));
        std::vector<std::pair<unsigned long long, uint32_t>> order;
        for (size_t i = 0; i < n_nodes; ++i)
            if (rank[i] != po::NODE_NO_RANK) order.emplace_back(rank[i], (uint32_t)i);
        std::sort(order.begin(), order.end());
        *n_out = order.size();
        for (size_t i = 0; i < order.size() && i < cap; ++i) nodes_out[i] = order[i].second;
    } catch (const std::bad_alloc&) {
        return fail(h, PO_ERR_NOMEM, "out of host memory in po_result_node_order");
    }
    return PO_OK;
}

// ---- diagnostics (tests/checker.py: GuardedReads) ------------------------------------------------------------------
uint64_t po_debug_host_ranges(uint64_t* out, uint64_t cap_entries) {
    std::lock_guard<std::mutex> lock(g_pin_mu);
    const uint64_t n = std::min<uint64_t>(cap_entries, g_pins.size());
    for (uint64_t i = 0; out && i < n; ++i) {
        out[3 * i] = g_pins[i].base;
        out[3 * i + 1] = g_pins[i].bytes;
        out[3 * i + 2] = g_pins[i].kind;
    }
    return g_pins.size();
}

uint64_t po_debug_store_words(const po_handle* h, int store, const uint64_t** words) {
    if (!h || store < 0 || store > 1) return 0;
    if (words) *words = h->words[store].data();
    return h->words[store].size();
}

// The host half of "rows home in compact form" on its own (no GPU): `n` records -> rows through the helper threads, exactly
// as po_overlaps_to_host runs them.  Returns 0, or the pool's error code (1 = the rows counted differ from n_rows_expected,
// 2 = a record names a read >= n_reads), -1 = no helper thread could be started.
int po_debug_expand_records(const po_cand* records, uint64_t n, const uint32_t* lengths, uint32_t n_reads, uint32_t paired,
                            po_row* rows_out, uint64_t n_rows_expected) {
    home::Pool* P = home::pool();
    if (!P) return -1;
    std::lock_guard<std::mutex> call(P->call_mu);
    home::begin(P, lengths, n_reads, false);
    home::Job j;
    j.rec = records;
    j.n_rec = n;
    j.out = rows_out;
    j.n_rows = n_rows_expected;
    j.paired = paired ? 1u : 0u;
    home::submit(P, j);
    home::wait_all(P);
    return P->error.load();
}

// ... the same for records of 8 bytes (po::pack_record with the shifts sh_b, sh_p: a | b << sh_b | p << sh_p | type << 62)
int po_debug_expand_packed(const uint64_t* records, uint64_t n, uint32_t sh_b, uint32_t sh_p, const uint32_t* lengths, uint32_t n_reads,
                           uint32_t paired, po_row* rows_out, uint64_t n_rows_expected) {
    if (!sh_b || sh_p < sh_b || sh_p >= 62) return -2;
    home::Pool* P = home::pool();
    if (!P) return -1;
    std::lock_guard<std::mutex> call(P->call_mu);
    home::begin(P, lengths, n_reads, false);
    home::Job j;
    j.rec = records;
    j.sh_b = sh_b;
    j.sh_p = sh_p;
    j.n_rec = n;
    j.out = rows_out;
    j.n_rows = n_rows_expected;
    j.paired = paired ? 1u : 0u;
    home::submit(P, j);
    home::wait_all(P);
    return P->error.load();
}

// SIGSEGV / SIGBUS: the faulting address and the NATIVE stack of the faulting thread to `fd`, then the handler that was
// installed before (Python's faulthandler prints Python frames only: a store by a runtime thread has none).
static int g_fault_fd = 2;
static struct sigaction g_fault_prev[2];
static void fault_handler(int sig, siginfo_t* si, void* ctx) {
    char line[128];
    const int n = std::snprintf(line, sizeof(line), "[phasm] signal %d at address %p (code %d); native stack of the faulting thread:\n", sig,
                                si ? si->si_addr : nullptr, si ? si->si_code : 0);
    if (n > 0) (void)!::write(g_fault_fd, line, (size_t)n);
    void* frames[64];
    const int k = backtrace(frames, 64);
    backtrace_symbols_fd(frames, k, g_fault_fd);
    const struct sigaction& prev = g_fault_prev[sig == SIGBUS ? 1 : 0];
    if ((prev.sa_flags & SA_SIGINFO) && prev.sa_sigaction) {
        prev.sa_sigaction(sig, si, ctx);
        return;
    }
    if (prev.sa_handler != SIG_DFL && prev.sa_handler != SIG_IGN && prev.sa_handler) {
        prev.sa_handler(sig);
        return;
    }
    signal(sig, SIG_DFL);
    raise(sig);
}

int po_debug_fault_backtrace(int fd) {
    g_fault_fd = fd;
    struct sigaction sa;
    std::memset(&sa, 0, sizeof(sa));
    sa.sa_sigaction = fault_handler;
    sa.sa_flags = SA_SIGINFO | SA_NODEFER;
    sigemptyset(&sa.sa_mask);
    void* warm[4];
    (void)backtrace(warm, 4);   // (loads libgcc now, not inside the handler)
    return (sigaction(SIGSEGV, &sa, &g_fault_prev[0]) == 0 && sigaction(SIGBUS, &sa, &g_fault_prev[1]) == 0) ? 0 : -1;
}

int po_debug_pointer_info(const void* p, int32_t* hip_type, int32_t* hsa_type, uint64_t* base, uint64_t* bytes) {
    if (hip_type) *hip_type = -1;
    if (hsa_type) *hsa_type = -1;
    if (base) *base = 0;
    if (bytes) *bytes = 0;
    if (!p) return 0;
    int known = 0;
    {
        hipPointerAttribute_t at;
        std::memset(&at, 0, sizeof(at));
        const hipError_t e = hipPointerGetAttributes(&at, p);
        if (e == hipSuccess) {
            if (hip_type) *hip_type = (int32_t)at.type;
            if (at.type != hipMemoryTypeUnregistered) known = 1;
        } else {
            (void)hipGetLastError();   // (an address the runtime has never heard of is an "invalid value" on older runtimes)
        }
    }
    {
        // the ROCr view: HIP's own pins of pageable copy sources / destinations (hsa_amd_memory_lock) show here too.
        // Resolved at run time from the HSA runtime the HIP runtime has loaded (this library links to HIP only).
        struct PtrInfo {   // hsa_amd_pointer_info_t (hsa_ext_amd.h)
            uint32_t size;
            uint32_t type;   // 0 unknown, 1 HSA allocation, 2 locked (registered host memory), 3 graphics, 4 IPC
            void* agentBaseAddress;
            void* hostBaseAddress;
            size_t sizeInBytes;
            void* userData;
            uint64_t agentOwner;
            uint32_t global_flags;
        };
        using Fn = int (*)(const void*, PtrInfo*, void* (*)(size_t), uint32_t*, void**);
        static Fn fn = reinterpret_cast<Fn>(dlsym(RTLD_DEFAULT, "hsa_amd_pointer_info"));
        if (fn) {
            PtrInfo info;
            std::memset(&info, 0, sizeof(info));
            info.size = sizeof(info);
            if (fn(p, &info, nullptr, nullptr, nullptr) == 0) {
                if (hsa_type) *hsa_type = (int32_t)info.type;
                if (info.type != 0) {
                    known = 1;
                    if (base) *base = (uint64_t)(uintptr_t)(info.hostBaseAddress ? info.hostBaseAddress : info.agentBaseAddress);
                    if (bytes) *bytes = info.sizeInBytes;
                }
            }
        }
    }
    return known;
}

po_status po_get_stats(const po_handle* h, po_stats* out) {
    if (!h || !out) return PO_ERR_INVALID;
    *out = h->stats;
    return PO_OK;
}

const char* po_last_error(const po_handle* h) { return h ? h->err.c_str() : "null handle"; }

}  // extern "C"
