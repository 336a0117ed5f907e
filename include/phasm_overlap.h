/* phasm_overlap.h -- C ABI of libphasm_overlap.so, the MI355X (gfx950) replacement for PHASM's
 * all-pairs exact read-overlap finder.
 *
 * What this boundary replaces.  The reference has no C ABI; its overlapper is a C++ class
 * exposed to Python through pybind11:
 *
 *   class ExactOverlapper                   /root/reference/src/overlapper.h:19-29
 *     ExactOverlapper()                     src/overlapper.cpp:19      (py::init,  src/phasm.cpp:13)
 *     addSequence(id, seq)                  src/overlapper.cpp:22-26   ("add_sequence", phasm.cpp:14)
 *     overlaps(min_length) -> vector<OverlapT>  src/overlapper.cpp:28-150 ("overlaps", phasm.cpp:15)
 *   OverlapT = tuple<string,string,int,int,int,int>                    src/overlapper.h:17
 *
 * Each entry point below names the reference interface it stands in for.  Only plain
 * pointers and sizes cross the boundary: no C++ types, no exceptions, no torch types.
 * Every function that can fail returns a po_status; po_last_error() has the message.
 *
 * There is no CPU fallback behind this ABI: every overlap is computed by the HIP kernels
 * in phasm_amd/csrc/.  Without a usable GPU, po_overlaps* fails with PO_ERR_HIP.
 *
 * Threading: one handle = one caller at a time (the reference object is not thread-safe
 * either).  Each handle owns one HIP stream and its device buffers.
 */
#ifndef PHASM_OVERLAP_H
#define PHASM_OVERLAP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PO_ABI_VERSION 4

typedef enum {
    PO_OK = 0,
    PO_ERR_INVALID = 1,  /* bad argument (NULL handle, shard >= nshards, ...)            */
    PO_ERR_NOMEM = 2,    /* host or device allocation failed  -> MemoryError in the shim */
    PO_ERR_HIP = 3,      /* HIP runtime error / no device     -> RuntimeError            */
    PO_ERR_CAPACITY = 4  /* candidate or row count exceeds what one call can hold        */
} po_status;

typedef struct po_handle po_handle;
typedef struct po_result po_result;

/* One overlap edge.  Same six fields as OverlapT (src/overlapper.h:17) with the two id
 * strings replaced by read indices (insertion order of po_add_sequence); ids are resolved
 * with po_get_id.  Coordinates are 0-based half-open on the oriented string as added;
 * bstart is always 0 (src/overlapper.cpp:81,110).                                         */
typedef struct {
    uint32_t a_idx, b_idx;
    int32_t astart, aend, bstart, bend;
} po_row;

/* Per-call device timings (HIP events on the handle's stream) and counters of the last
 * po_overlaps* call on this handle; feeds bench.py's roofline object.                     */
typedef struct {
    uint32_t bits_per_base;      /* 2 (pure ACGT) or 8 (raw bytes)                          */
    uint32_t kmer;               /* anchor length K = min(64/bits, max(min_length,1))       */
    uint32_t paired;             /* 1: reads are (x, revcomp x) pairs -> one member of each  */
    uint32_t wide_index;         /*    strand-mirror pair verified, the other row mirrored.  */
                                 /* wide_index 1: W K-mers per read indexed, word-aligned      */
                                 /*    probes only (large read sets); 0: prefix + LDS filter  */
    uint64_t n_reads;            /* reads in the handle                                     */
    uint64_t n_eligible;         /* reads with length >= min_length (can be a `b`)          */
    uint64_t total_bases;        /* sum of read lengths (oriented bases B)                  */
    uint64_t shard_bases;        /* bases of the a-side reads scanned by this call          */
    uint64_t n_tiles;            /* 64-word scan tiles in this call's shard                 */
    uint64_t n_candidates;       /* anchor hits (a, p, b) handed to the verify kernel       */
    uint64_t n_verified;         /* candidates that verified                                */
    uint64_t n_rows;             /* rows emitted (A + B, duplicates included)               */
    uint64_t sum_overlap_bases;  /* sum over emitted rows of the overlap length l           */
    uint64_t verify_bytes_algo;  /* sum over emitted rows of 2*ceil(l*bits/8) (both sides)  */
                                 /* Stage times come from events recorded between the kernels (~5 us of device time     */
                                 /* each).  A streamed step (streamed == 1) records only the pairs around its two big   */
                                 /* kernels: ms_index .. ms_emit are 0 there, ms_total, ms_scan_probe and               */
                                 /* ms_verify_kernel are sums over the pieces; PHASM_PHASE_EVENTS=1 records them all.   */
    float ms_index;              /* anchor table + chains + Bloom filter build              */
    float ms_scan_count;         /* position scan, counting pass                            */
    float ms_scan_fill;          /* position scan, candidate fill pass                      */
    float ms_verify;             /* packed exact verify of all candidates                   */
    float ms_select;             /* longest-only selection + row counting                   */
    float ms_emit;               /* row emission                                            */
    float ms_total;              /* first kernel start -> last kernel end                   */
    float ms_upload;             /* H2D of the packed read set if this call uploaded it     */
    float ms_scan_probe;         /* the scan kernel alone (k_scan_probe / k_wide_scan count pass), inside ms_scan_count */
    float ms_verify_kernel;      /* the verify kernel alone (k_verify_a), inside ms_verify; 0 when there was nothing to verify */
    uint64_t verify_bytes_exec;  /* sum over the VERIFIED CANDIDATES of 2*ceil(n*bits/8): the bytes the verify kernel  */
                                 /* really compared (a strand-mirror pair is compared once and emitted twice)        */
    uint64_t dp_steps;           /* po_overlaps_ex: antidiagonals swept by the DP kernel, summed over the candidates */
    uint64_t dp_stopped;         /*                 candidates whose whole band rose above max_diff before the end   */
    uint32_t max_diff, band;     /*                 the parameters of the call (0, 0 for the exact entry points)     */
    uint32_t index_reused;       /* 1: the anchor index of the previous call on this handle was reused (same upload,   */
    uint32_t dp_lanes;           /*    same min_length and flavour); 0: built in this call.  dp_lanes (po_overlaps_ex):  */
                                 /*    2 = lane per candidate, band row as a bit vector; 1 = lane per candidate, band row */
                                 /*    in registers; 0 = wave per candidate (a lane per diagonal)                         */
    uint64_t upload_bytes;       /* bytes the last po_upload moved host->device (half the packed set when every   */
                                 /* odd read is the reverse complement of its even partner: the device rebuilds them) */
    uint32_t streamed;           /* po_overlaps_to_host: 1 = streamed step (reads uploaded piece by piece under the      */
    uint32_t n_deferred;         /*    kernels); n_deferred = containment candidates that waited for a later piece       */
                                 /*    (streamed == 0 with n_deferred > 0: their list overflowed, the chunked form ran)  */
    uint32_t fused_tail;         /* chunks / pieces of the call whose select + row offsets + emission ran as ONE kernel   */
    uint32_t tail_fallback;      /*    (k_tail: needs a kept row buffer that holds the worst case); tail_fallback = how   */
                                 /*    often that kernel met tandem-repeat reads and the classic kernels ran instead      */
    uint32_t n_predicted;        /* streamed step: pieces whose candidate count was predicted from the previous call on   */
    uint32_t home_record_bytes;  /*    the same reads (no host round trip between the counting pass and the rest).        */
                                 /* home_record_bytes (po_overlaps_to_host): what crossed PCIe per strand-mirror pair of  */
                                 /*    rows -- 8 or 16 (a verified-candidate record, the host wrote the rows), 0 = the rows */
} po_stats;

/* ExactOverlapper()  -- src/overlapper.cpp:19, py::init at src/phasm.cpp:13. */
po_status po_create(po_handle** out);
void po_destroy(po_handle* h);

/* Choose the HIP device (default 0).  Call it BEFORE adding reads: once the read set is large (64 M bases) the library
 * brings the device up while reads are still being added -- runtime start, stream, a pinned result pool sized from
 * the bases seen so far -- so that the first po_overlaps* call does not pay for it; after that a different device is
 * refused (PO_ERR_INVALID). */
po_status po_set_device(po_handle* h, int device);

/* addSequence(id, seq)  -- src/overlapper.cpp:22-26.  Copies id and seq (the caller may
 * free them at once).  seq is compared byte-wise, like the reference's CharString.  Reads are
 * stored at 2 bits per base; bytes other than upper-case A/C/G/T (N, IUPAC codes, lower case) are
 * kept as sparse exception records beside the 2-bit codes and compared exactly after the packed
 * compare.  Only when such bytes are dense (more than len/64 + 16 in one read) does the whole handle
 * move to the slower 8-bits-per-base representation.                                        */
po_status po_add_sequence(po_handle* h, const char* id, size_t id_len, const char* seq, size_t seq_len);

/* FASTA ingest for `phasm overlap` (the reference uses dinopy.FastaReader / dinopy.reverse_complement,
 * phasm/cli/assembler.py:32-40): the record name is the whole header line, sequence lines are joined,
 * blank lines skipped.  both_strands != 0 adds every record as name+"+" / sequence and name+"-" /
 * reverse complement, exactly what the CLI feeds the overlapper (:38-40). */
po_status po_add_fasta(po_handle* h, const char* path, int both_strands, uint64_t* n_records);

uint32_t po_num_sequences(const po_handle* h);
po_status po_get_id(const po_handle* h, uint32_t idx, const char** id, size_t* id_len);
uint32_t po_get_length(const po_handle* h, uint32_t idx);

/* Pack (if needed) and copy the read set to the device now instead of at the first
 * po_overlaps* call.  Idempotent until the next po_add_sequence.                          */
po_status po_upload(po_handle* h);

/* Sharded upload for multi-GPU jobs.  Every rank needs the whole read set in its HBM (any read can be a `b`), but not
 * over its own PCIe link: rank g copies only the words of shard g's even reads host->device, into its slot of an
 * exchange buffer (po_upload_piece; dst_device == NULL just asks for the piece's length), one all-gather over xGMI hands
 * every rank all pieces (phasm_amd/dist.py: ReadExchange), and po_upload_assemble puts them in place and finishes the
 * upload (odd reads rebuilt on the device, tiles, tables).  *ok = 0: the reads are not (x, reverse complement of x)
 * pairs -- use po_upload.  The reference has no counterpart (one process, reads already in host memory). */
po_status po_upload_piece(po_handle* h, uint32_t shard, uint32_t nshards, void* dst_device, uint64_t capacity_words,
                          uint64_t* word_count, int* ok);
po_status po_upload_assemble(po_handle* h, const void* pieces_device, uint64_t slot_words, uint32_t nshards);
/* The same in `nparts` parts per shard (equal chunks of the shard's piece): the host->device copy of part k + 1 runs while
 * the all-gather of part k is in flight.  The gathered buffer handed to po_upload_assemble_parts is laid out
 * [part][shard][slot_words]. */
po_status po_upload_piece_part(po_handle* h, uint32_t shard, uint32_t nshards, uint32_t part, uint32_t nparts, void* dst_device,
                               uint64_t capacity_words, uint64_t* word_count, int* ok);
po_status po_upload_assemble_parts(po_handle* h, const void* pieces_device, uint64_t slot_words, uint32_t nshards, uint32_t nparts);

/* Forget the device copy of the read set: the next po_upload / po_overlaps* copies the packed reads host->device
 * again, as the first call of a fresh process does.  The reference's overlaps() starts from the host-side string
 * set on every call (index built from `readset`, src/overlapper.cpp:33-36), so ONE reference call corresponds to
 * po_invalidate + po_overlaps_to_host + po_result_rows: the region bench.py times. */
po_status po_invalidate(po_handle* h);

/* overlaps(min_length)  -- src/overlapper.cpp:28-150.  Rows stay on the device until po_result_rows() is called.
 * Same rows on every call, like the reference.  The reference rebuilds its index inside every call (:33-36); this
 * library does so whenever the device copy of the reads has changed (po_add_*, po_invalidate: what a reference call
 * always faces) and otherwise REUSES the anchor index it built for the same upload, min_length and flavour
 * (po_stats.index_reused = 1; PHASM_NO_INDEX_REUSE=1 rebuilds per call).  min_length 0 behaves as 1 (a suffix array
 * has no empty suffix).  A handle also keeps its device workspaces, the pinned result buffers and -- for the streamed
 * form of po_overlaps_to_host -- the candidate counts per piece of the previous call on the same reads.              */
po_status po_overlaps(po_handle* h, uint32_t min_length, po_result** out);

/* overlaps(min_length) the way the reference returns it -- the whole vector<OverlapT> in host memory
 * (src/overlapper.cpp:149) -- as ONE pipelined call: po_overlaps + po_result_rows, with the rows of one chunk of a-side
 * reads travelling device->host (second stream, one page-locked array) while the next chunk is in the kernels.  The
 * result holds the host array only (po_result_rows returns it at once; po_result_device_rows is NULL; po_layout_edges
 * would copy the rows back).  Same multiset of rows as po_overlaps, a-major chunk by chunk.
 * When the read set changed since the last upload -- what the reference faces on every call, its reads are host memory
 * (:22-36) -- the call also does the upload, STREAMED: the packed reads cross PCIe in pieces on a third stream, a piece
 * that has landed is scanned against the whole index (built from every read's first two words, sent ahead), its candidates
 * whose b-side read has arrived are verified and emitted (every suffix-prefix candidate, by the choice of which member
 * of a strand-mirror pair is computed; containments of a read still on its way wait on a list), and its rows travel
 * home while the next piece is still coming in.  Needs reads added as (x, reverse complement of x) pairs of pure
 * upper-case ACGT; otherwise the call uploads first (po_upload) and runs the chunked form.
 * po_stats.streamed tells which form ran. */
po_status po_overlaps_to_host(po_handle* h, uint32_t min_length, po_result** out);

/* Banded seed-extension mode -- an EXTENSION BEYOND THE REFERENCE, which is exact (src/overlapper.cpp:28-150; CLI help
 * "exact overlaps", phasm/cli/assembler.py:436-439).  Same anchors as po_overlaps (b's K-base prefix found in a); every
 * candidate is extended by a banded edit-distance DP (unit costs, diagonals -band..band, band <= 30, one wavefront per
 * candidate: phasm_amd/csrc/extend.hip.h) and accepted with at most max_diff differences:
 *   A  all of a[p:] against a prefix of b  -> row (a, b, p, len(a), 0, bend)
 *   B  all of b against a prefix of a[p:]  -> row (a, b, p, aend, 0, len(b))
 * longest-only for A per ordered pair, every B occurrence, as in the exact contract.  max_diff = 0 returns exactly the
 * rows of po_overlaps (checked against the reference goldens); max_diff > 0 has no reference counterpart -- its checker
 * is the build's own CPU restatement, oracle/extend_oracle.c, itself held against an independent definition and rows
 * known by construction (tests/test_extend_definition.py).  Needs pure ACGT (2-bit) or 8-bit reads when max_diff > 0,
 * and always anchors on the prefix K-mer (the narrow index), whatever the size of the read set. */
po_status po_overlaps_ex(po_handle* h, uint32_t min_length, uint32_t max_diff, uint32_t band, po_result** out);

/* Multi-GPU form: only the rows whose `a` read lies in shard `shard` of `nshards` (contiguous
 * read-index ranges balanced by base count) are produced.  The union over all shards is
 * exactly the po_overlaps() result; the caller merges (RCCL all-gather in phasm_amd/dist.py). */
po_status po_overlaps_shard(po_handle* h, uint32_t min_length, uint32_t shard, uint32_t nshards,
                            po_result** out);

/* Multi-GPU exchange in compact form.  po_candidates_shard: like po_overlaps_shard, but the result
 * holds the shard's VERIFIED CANDIDATES as po_cand[po_result_count] (16 B each; in paired-strand mode
 * one per strand-mirror pair) instead of rows (24 B each, both members): 3-4x fewer bytes over xGMI.
 * Read it with po_result_device_rows / po_result_copy_to_device (or po_result_rows cast to po_cand*).
 * po_expand: turn a candidate array on this handle's device -- normally the rank-order concatenation
 * of every shard's candidates -- into rows: exactly the po_overlaps() rows (as a multiset; the emission order
 * follows the candidate array).  All-zero entries are padding and skipped (RCCL has no all-gatherv: the
 * shards travel in equal-sized slots); any other entry this library could not have produced is an error. */
typedef struct {
    uint32_t a_idx, p, b_idx, type; /* type bit0: A row (suffix of a = prefix of b), bit1: B row (b inside a) */
} po_cand;
po_status po_candidates_shard(po_handle* h, uint32_t min_length, uint32_t shard, uint32_t nshards, po_result** out);
po_status po_expand(po_handle* h, const void* candidates_device, uint64_t n_candidates, po_result** out);
/* po_candidates_shard with the destination supplied: when the shard's candidates fit `capacity` entries they are
 * written straight to dst_device (e.g. this rank's slot of the exchange buffer; *written = 1, the result carries
 * the count and points at dst_device); otherwise *written = 0 and the result holds them as usual. */
po_status po_candidates_shard_into(po_handle* h, uint32_t min_length, uint32_t shard, uint32_t nshards,
                                   void* dst_device, uint64_t capacity, int* written, po_result** out);

/* Sliced wide index: the part of a multi-GPU step that used to be replicated.  Large read sets (> 160 k reads of
 * length >= min_length) use the wide index (W K-mers per read, GBs of table at config 5), and every rank used to build
 * all of it.  Here the table is n_slices sub-tables by key hash; rank g builds sub-table g only (po_index_slice_build),
 * copies it and its chain segment into its slot of an exchange buffer (po_index_slice_export: chunk layout and size
 * from po_index_chunk_bytes), the chunks travel in ONE all-gather (phasm_amd/dist.py: IndexExchange), and the shard
 * call probes the gathered index (po_candidates_shard_indexed) instead of building one.  *is_wide = 0 means this read
 * set uses the narrow index (0.06 ms to build: not worth exchanging) -- call po_candidates_shard as before.  The
 * reference has no counterpart (one process: overlapper.cpp:33-36 builds one suffix array). */
po_status po_index_slice_build(po_handle* h, uint32_t min_length, uint32_t slice, uint32_t n_slices, uint32_t* is_wide,
                               uint32_t* slice_bits, uint64_t* chain_entries);
uint64_t po_index_chunk_bytes(uint32_t slice_bits, uint64_t chain_capacity, uint64_t* chain_offset_bytes);
po_status po_index_slice_export(po_handle* h, void* dst_device, uint64_t chain_capacity);
po_status po_candidates_shard_indexed(po_handle* h, uint32_t min_length, uint32_t shard, uint32_t nshards,
                                      const void* index_device, uint32_t n_slices, uint32_t slice_bits, uint64_t chain_capacity,
                                      void* dst_device, uint64_t capacity, int* written, po_result** out);
po_status po_overlaps_shard_indexed(po_handle* h, uint32_t min_length, uint32_t shard, uint32_t nshards, const void* index_device,
                                    uint32_t n_slices, uint32_t slice_bits, uint64_t chain_capacity, po_result** out);

/* The read-index range [*r_begin, *r_end) that po_overlaps_shard(shard, nshards) scans on the
 * a-side.  Pure host logic (no GPU needed). */
po_status po_shard_range(const po_handle* h, uint32_t shard, uint32_t nshards, uint32_t* r_begin, uint32_t* r_end);

uint64_t po_result_count(const po_result* r);
/* Host pointer to po_result_count() rows (copied device->host on first use, into page-locked memory owned by the
 * library: one DMA, valid until po_result_free); NULL on error.  The counterpart of the reference returning its
 * vector<OverlapT> to the host (src/overlapper.cpp:149). */
const po_row* po_result_rows(po_result* r);
/* Host pointer to rows [first, first + count) only (one rank's share of a merged multi-GPU result: the ranks of a node
 * bring the rows home once between them).  Valid until the next call on the handle; NULL on error or count == 0. */
const po_row* po_result_rows_range(po_result* r, uint64_t first, uint64_t count);
/* Device pointer to the same rows (valid until po_result_free). */
const void* po_result_device_rows(const po_result* r);
/* Copy the rows device->device into dst (>= count*sizeof(po_row) bytes), e.g. a torch tensor. */
po_status po_result_copy_to_device(po_result* r, void* dst_device);
/* The same for the first `count` entries only (count <= po_result_count). */
po_status po_result_copy_prefix_to_device(po_result* r, void* dst_device, uint64_t count);
void po_result_free(po_result* r);

/* Write one GFA2 edge line per row to the file descriptor, byte-identical to the reference's
 * gfa_line("E", "*", a_id, b_id, astart, aend, bstart, bend, "*")  (assembler.py:46-48, gfa.py:230-231).  The lines go
 * behind the descriptor's position, in row order, whatever the descriptor is: a regular file opened without O_APPEND is
 * written in parallel at computed offsets, anything else (a pipe, a descriptor opened for appending) in order. */
po_status po_write_gfa_edges(po_result* r, int fd, uint64_t* lines_out);
/* The segment lines that go before them: `S <name> <length> *` per read pair (assembler.py:38; the handle's reads
 * must have been added as name+"+" / name+"-" pairs). */
po_status po_write_gfa_segments(po_handle* h, int fd, uint64_t* lines_out);
/* (Given a po_layout_edges result instead, the same call writes the graph's edges the way the reference's
 * graph writer does: `E * <u> <v> <weight> <len(u)> 0 <overlap_len> *`, gfa2_write_graph, gfa.py:315-327.) */

/* ---------------------------------------------------------------------------------------------
 * Next row of the path: the consumer of the E lines, stage 1 of
 * `phasm layout` (phasm/cli/assembler.py:52-139) -- classify every alignment, drop contained reads,
 * apply the alignment filters, build the assembly-graph edge list -- on the row array, on the device.
 * --------------------------------------------------------------------------------------------- */

/* The filter settings of `phasm layout` (assembler.py:78-87; CLI defaults :469-489). */
typedef struct {
    uint32_t min_read_length;    /* MinReadLength(n), phasm/filter.py:37-58; 0 = filter not installed  */
    uint32_t min_overlap_length; /* MinOverlapLength(n), filter.py:61-74;   0 = filter not installed  */
    uint32_t max_overhang_abs;   /* MaxOverhang(max_overhang, ratio), filter.py:104-122; default 1000 */
    uint32_t reserved;           /* must be 0                                                         */
    double max_overhang_rel;     /* default 0.8                                                       */
} po_layout_params;

/* One assembly-graph edge: g.add_edge(u, v, {weight, overlap_len}), phasm/assembly_graph.py:146-176.
 * u, v are oriented-read indices of the handle (x+ = 2i, x- = 2i+1; reverse node = index ^ 1). */
typedef struct {
    uint32_t u, v;
    int32_t weight, overlap_len;
} po_edge;

typedef struct {
    uint64_t n_rows;             /* alignments looked at                                              */
    uint64_t n_type[4];          /* rows per AlignmentType (phasm/alignments.py:16-20):               */
                                 /*   0 OVERLAP_AB, 1 OVERLAP_BA, 2 A_CONTAINED, 3 B_CONTAINED         */
    uint64_t n_short;            /* overlap rows with a read shorter than min_read_length             */
    uint64_t n_min_overlap;      /* ... then: shorter than min_overlap_length                         */
    uint64_t n_overhang;         /* ... then: overhang above the MaxOverhang threshold                */
    uint64_t n_pass;             /* overlap rows that satisfy all three predicates                    */
    uint64_t n_contained_reads;  /* reads (both strands count once) that are contained in another     */
    uint64_t n_edges;            /* distinct (u, v) edges of the graph after the contained reads left */
    float ms_classify, ms_dedupe, ms_emit, ms_total;
} po_layout_stats;

/* A read without sequence: one GFA2 segment line `S <name> <length> *` (gfa2_segment_to_read,
 * phasm/io/gfa.py:33-46).  Adds the two oriented nodes name+"+" and name+"-" of that length.  A handle
 * holds either sequences or segments, never both; po_overlaps* on a segment handle fails. */
po_status po_add_segment(po_handle* h, const char* name, size_t name_len, uint32_t length);

/* Wrap rows supplied by the caller (copied) into a result of this handle, e.g. alignments from
 * another producer of the same wire format (phasm/cli/convert.py:65-133). */
po_status po_result_from_rows(po_handle* h, const po_row* rows, uint64_t n, po_result** out);

/* Read a GFA2 file the way `phasm layout` does (assembler.py:56-60, :96-98): pass 1 takes every S line
 * (gfa2_parse_segments, phasm/io/gfa.py:107-109) into an EMPTY handle via po_add_segment, pass 2 turns
 * every E line into a row (gfa2_parse_edge + gfa2_line_to_la, gfa.py:72-104: ids end in the strand
 * character, positions may carry a trailing `$`).  An E line naming an unknown segment fails, as the
 * reference's dict lookup does.  After a failure the handle may already hold some of the segments: destroy it. */
po_status po_add_gfa(po_handle* h, const char* path, uint64_t* n_segments, po_result** rows_out);

/* Stage 1 of `phasm layout` on the rows of `rows` (a result of this handle):
 *   1. classify each row (LocalAlignment.classify, phasm/alignments.py:248-258);
 *   2. ContainedReads (filter.py:77-101): the contained read of every *_CONTAINED row is marked;
 *   3. MinReadLength / MinOverlapLength / MaxOverhang on the remaining rows (filter.py:37-74, 104-122);
 *   4. build_assembly_graph (assembly_graph.py:136-179): two edges per surviving row; a later row
 *      overwrites the attributes of an edge an earlier row added (networkx add_edge);
 *   5. every marked read loses both of its nodes and their edges (assembler.py:113-126).
 * `edges_out` holds po_edge[po_result_count] (read with po_result_rows cast to const po_edge*, or the
 * device pointer), ordered by producing row.  The edge SET equals the reference's `g.edges(data=True)`
 * at "Final graph" (assembler.py:136) for any order of the input lines; the reference's per-filter
 * `filtered` log counters depend on line order and are not reproduced.
 * removed_reads_out (may be NULL): po_num_sequences()/2 bytes, 1 = read i (nodes 2i, 2i+1) was contained.
 * Needs the handle's ids in strand pairs (2i = name+"+", 2i+1 = name+"-", what po_add_fasta with
 * both_strands, the CLI and po_add_segment produce); otherwise PO_ERR_INVALID. */
po_status po_layout_edges(po_handle* h, po_result* rows, const po_layout_params* params,
                          uint8_t* removed_reads_out, po_result** edges_out);
po_status po_get_layout_stats(const po_handle* h, po_layout_stats* out);

/* ---------------------------------------------------------------------------------------------
 * The first two operations of stage 2 of `phasm layout` (phasm/cli/assembler.py:145-159) on the
 * edges po_layout_edges left on the device: transitive reduction, then the symmetry pass.
 * --------------------------------------------------------------------------------------------- */

typedef struct {
    int32_t length_fuzz;         /* remove_transitive_edges(g, length_fuzz); CLI default 1000, assembler.py:504 */
    uint32_t reserved;           /* must be 0                                                         */
} po_reduce_params;

typedef struct {
    uint64_t n_edges_in;         /* edges of the stage-1 graph                                        */
    uint64_t n_transitive;       /* "Removing %d transitive edges...", assembler.py:157                */
    uint64_t n_asymmetric;       /* edges make_symmetric removed after that, assembler.py:159         */
    uint64_t n_edges_out;        /* edges left                                                        */
    uint64_t max_out_degree;     /* longest adjacency list of the stage-1 graph                       */
    float ms_csr, ms_mark, ms_symmetric, ms_emit, ms_total;
} po_reduce_stats;

/* `edges` is a po_layout_edges result of this handle; it stays valid and unchanged (reduce it again with
 * another fuzz).  In order:
 *   1. sort_adjacency_lists (phasm/assembly_graph.py:48-55, :211): every adjacency list ascending by weight,
 *      ties in the order the reference's OrderedDict holds them -- by the FIRST input row that wrote the edge
 *      (networkx's add_edge on an existing edge keeps its position);
 *   2. remove_transitive_edges (assembly_graph.py:215-262) per node v: all neighbours IN_PLAY; sequentially over
 *      w in adj[v], skipping a w that is no longer IN_PLAY, every IN_PLAY x in adj[w] with
 *      weight(v,w) + weight(w,x) <= weight(v, last neighbour) + length_fuzz is ELIMINATED; then for every w the
 *      first entry of adj[w] and every x with weight(w,x) < length_fuzz is ELIMINATED; (v, w) is transitive iff
 *      w ended ELIMINATED.  Plain signed integers; weights may be <= 0;
 *   3. g.remove_edges_from (assembler.py:158);
 *   4. make_symmetric (assembly_graph.py:429-443): one pass, (u, v) goes iff (v^1, u^1) is no longer an edge.
 * edge_flags_out (may be NULL): po_result_count(edges) bytes, one per stage-1 edge in its order -- 0 kept,
 * 1 transitive (the reference's TransitiveReduction metadata record, assembler.py:147-155), 2 removed by the
 * symmetry pass.  kept_out holds the kept po_edge entries in stage-1 order, an edge result like its input.
 * There is no CPU fallback: without a GPU the call returns PO_ERR_HIP.  A result of another handle, a result that
 * is not a po_layout_edges result, reserved != 0 or length_fuzz < 0: PO_ERR_INVALID.  kept_out carries the node order
 * of its input on (po_result_node_order).  Tip removal follows with po_layout_tips. */
po_status po_layout_reduce(po_handle* h, po_result* edges, const po_reduce_params* params, uint8_t* edge_flags_out,
                           po_result** kept_out);
po_status po_get_reduce_stats(const po_handle* h, po_reduce_stats* out);

/* ---------------------------------------------------------------------------------------------
 * The next three calls of stage 2 (phasm/cli/assembler.py:161-167, and again :177-179):
 * remove_tips, make_symmetric, clean_graph, on an edge result of this handle.
 * --------------------------------------------------------------------------------------------- */

typedef struct {
    uint32_t max_tip_len;        /* remove_tips(g, max_tip_len, ...); CLI default 4, assembler.py -t            */
    int32_t max_tip_len_bases;   /* ... max_tip_len_bases; CLI and function default 5000                         */
    uint32_t reserved;           /* must be 0                                                                    */
} po_tips_params;

typedef struct {
    uint64_t n_edges_in;         /* edges of the input graph                                                     */
    uint64_t n_in_tip_edges;     /* edges remove_incoming_tips removed (assembly_graph.py:326-381)                */
    uint64_t n_out_tip_edges;    /* edges remove_outgoing_tips removed (:267-323)                                 */
    uint64_t n_asymmetric;       /* edges make_symmetric removed after that                                      */
    uint64_t n_edges_out;        /* edges left                                                                   */
    uint64_t n_nodes;            /* nodes of the input graph (those in its node order)                           */
    uint64_t n_isolated_nodes;   /* nodes clean_graph removed: no edge left                                      */
    uint64_t n_candidates_in;    /* nodes with in-degree 0 and out-degree 1 at the start of the incoming pass    */
    uint64_t n_candidates_out;   /* nodes with out-degree 0 and in-degree 1 at the start of the outgoing pass    */
    uint64_t n_rounds_in;        /* rounds the device needed to settle the candidates in node order              */
    uint64_t n_rounds_out;
    float ms_setup, ms_incoming, ms_outgoing, ms_symmetric, ms_emit, ms_total;
} po_tips_stats;

/* `edges` is an edge result of this handle -- from po_layout_edges, the kept_out of po_layout_reduce or the kept_out
 * of this call; it stays valid and unchanged.  The graph's nodes are those in the result's node order (below); a
 * node without edges is a node until this call counts it as isolated.  In order:
 *   1. remove_incoming_tips: tips = the nodes with in-degree 0 at the start, in node order.  For each tip s with
 *      out-degree 1, on the graph as the tips before it left it: path = [s]; while out(curr) == 1 and in(curr) <= 1
 *      the one successor is appended and becomes curr, and the edge's weight joins a signed 64-bit sum; a path of more
 *      than max_tip_len + 1 nodes, or a sum above max_tip_len_bases, is no tip.  If the loop ends by its own condition
 *      every edge of the path goes, the last one into the junction or dead end included;
 *   2. remove_outgoing_tips: the same on the reversed graph (tips = nodes with out-degree 0, predecessors walked);
 *   3. make_symmetric: one pass, (u, v) goes iff (v^1, u^1) is no longer an edge;
 *   4. clean_graph: the nodes left without an edge are counted and leave the node order of kept_out.
 * The result depends on the node order, as the reference's does; the device reproduces it exactly.
 * edge_flags_out (may be NULL): po_result_count(edges) bytes in input order -- 0 kept, 1 incoming-tip edge,
 * 2 outgoing-tip edge, 3 removed by the symmetry pass.  kept_out holds the kept edges in input order.
 * There is no CPU fallback: without a GPU the call returns PO_ERR_HIP.  A result of another handle, a result that
 * is no edge result, reserved != 0: PO_ERR_INVALID.  Diamond tips follow with po_layout_diamonds, the merging
 * of unambiguous paths with po_layout_merge, the average coverage per edge with po_layout_coverage; of `phasm chain`
 * this library has the weakly connected components (po_layout_components), the partition that superbubble detection
 * starts with (po_layout_partition), the superbubbles of the acyclic partitions (po_layout_superbubbles), the bubble
 * chains built from them (po_layout_bubblechains) and the contigs outside the chains (po_layout_contigs); of `phasm phase`
 * the scoring and pruning of the haplotype extensions at one bubble (po_phase_branch) and the relevant reads of a bubble
 * (po_phase_index, po_phase_relevant).  The superbubbles of the cyclic partitions (what the reference reaches through
 * graph_to_dag) come from po_layout_superbubbles_all, by a scheme of its own; the chains, contigs and paths still take the
 * acyclic partitions only. */
po_status po_layout_tips(po_handle* h, po_result* edges, const po_tips_params* params, uint8_t* edge_flags_out,
                         po_result** kept_out);
po_status po_get_tips_stats(const po_handle* h, po_tips_stats* out);

/* ---------------------------------------------------------------------------------------------
 * The call between the two tip blocks of stage 2 (phasm/cli/assembler.py:173): remove_diamond_tips
 * (phasm/assembly_graph.py:721-743) on an edge result of this handle.
 * --------------------------------------------------------------------------------------------- */

typedef struct {
    uint32_t reserved;           /* must be 0                                                                    */
} po_diamond_params;

typedef struct {
    uint64_t n_edges_in;         /* edges of the input graph                                                     */
    uint64_t n_edges_out;        /* edges left: n_edges_in - 3 * n_diamonds                                      */
    uint64_t n_nodes;            /* nodes of the input graph (those in its node order)                           */
    uint64_t n_nodes_removed;    /* end nodes and pred1 nodes that left the graph: 2 * n_diamonds                */
    uint64_t n_candidates;       /* nodes with out-degree 0 and in-degree 2 at the start                         */
    uint64_t n_diamonds;         /* "Removed %d diamond tips", assembler.py:174                                  */
    uint64_t n_rounds;           /* rounds the device needed to settle the candidates in node order              */
    uint64_t n_invalid;          /* edges that name a read the handle does not hold (the call fails then)        */
    float ms_setup, ms_rounds, ms_emit, ms_total;
} po_diamond_stats;

/* `edges` is an edge result of this handle -- from po_layout_edges, po_layout_reduce, po_layout_tips or this call; it
 * stays valid and unchanged, its node order too.  end_nodes = the nodes with out-degree 0 and in-degree 2 at the start,
 * in node order.  For each end node E, on the graph as the end nodes before it left it: among its two predecessors,
 * pred1 is one with out-degree 1 and in-degree 1 and gt1 one with out-degree > 1; if both exist, E and pred1 are removed
 * as NODES (one diamond): the two in-edges of E and the in-edge of pred1 go.  No symmetry pass and no clean_graph follow:
 * a node left without an edge stays in the node order of kept_out (the next po_layout_tips counts it as isolated).  The
 * result depends on the node order, as the reference's does; the device reproduces it exactly.
 * params may be NULL.  edge_flags_out (may be NULL): po_result_count(edges) bytes in input order -- 0 kept, 1 in-edge of
 * a removed end node, 2 the in-edge of a removed pred1.  kept_out holds the kept edges in input order and the node order
 * of the input without the removed nodes.  There is no CPU fallback: without a GPU the call returns PO_ERR_HIP.  A result
 * of another handle, a result that is no edge result, reserved != 0: PO_ERR_INVALID. */
po_status po_layout_diamonds(po_handle* h, po_result* edges, const po_diamond_params* params, uint8_t* edge_flags_out,
                             po_result** kept_out);
po_status po_get_diamond_stats(const po_handle* h, po_diamond_stats* out);

/* ---------------------------------------------------------------------------------------------
 * The last call of stage 2 that changes the graph before `phasm layout` writes it (phasm/cli/assembler.py:184-186):
 * merge_unambiguous_paths (phasm/assembly_graph.py:456-541) on an edge result of this handle.
 * --------------------------------------------------------------------------------------------- */

typedef struct {
    uint32_t reserved;           /* must be 0                                                                    */
} po_merge_params;

typedef struct {
    uint64_t n_edges_in;         /* edges of the input graph                                                     */
    uint64_t n_edges_out;        /* edges left: n_edges_in - (n_nodes_merged - n_merged)                         */
    uint64_t n_nodes;            /* nodes of the input graph (those in its node order)                           */
    uint64_t n_merged;           /* merged nodes K                                                               */
    uint64_t n_nodes_merged;     /* "Merged %d nodes.", assembler.py:186                                         */
    uint64_t max_path_nodes;     /* nodes of the longest path                                                    */
    uint64_t n_self_loops;       /* merged nodes that got a self-loop from the edge (last node -> head)          */
    uint64_t n_cycle_nodes;      /* nodes with a link in and out that reached no head (they stay as they are)    */
    uint64_t n_rounds;           /* pointer-jumping rounds run: at most ceil(log2(n_nodes)) + 1                  */
    uint64_t n_overflow;         /* weights that do not fit int32 / ids that do not fit uint32 (the call fails)  */
    uint64_t n_invalid;          /* edges that name a read the handle does not hold (the call fails then)        */
    float ms_links, ms_rank, ms_number, ms_emit, ms_total;
} po_merge_stats;

/* `edges` is an edge result of this handle -- from po_layout_edges, po_layout_reduce, po_layout_tips or
 * po_layout_diamonds; it stays valid and unchanged, its node order too.  With distinct edges (u, v, weight, overlap_len):
 * link(u) = v iff u has one out-edge, into v, and v has one in-edge.  A head is a node with a link out and none in; its
 * path is the head followed by its links (at least two nodes).  Nodes on cycles of links stay as they are.  Paths are
 * numbered k = 0, 1, ... by the rank of their head in the node order (the reference's "merged%d", strand +).  An input
 * edge that is a link of a path goes.  Every other edge (u, v) stays, in input order: u on a path (its last node) is
 * renamed to the merged node and weight += the sum of the path's link weights; v on a path (its head) is renamed;
 * overlap_len stays.  Merged node k is written as n_nodes + k, n_nodes = po_num_sequences(h).  An edge from a path's last
 * node to its own head becomes a self-loop of the merged node.  The node order of merged_out: the unmerged nodes in their
 * old order, then the merged nodes by k.
 * params may be NULL.  edge_flags_out (may be NULL): po_result_count(edges) bytes in input order -- 0 kept as it is,
 * 1 link of a path (gone), 2 kept with a renamed end or a raised weight.  merged_out is a MERGED GRAPH: po_result_count,
 * po_result_rows and po_result_node_order work on it; po_layout_reduce, _tips, _diamonds and _merge refuse it with
 * PO_ERR_INVALID (their kernels index by oriented read).  A weight that does not fit int32 or an id that does not fit
 * uint32: PO_ERR_INVALID and n_overflow > 0, never a wrapped value.  There is no CPU fallback: without a GPU the call
 * returns PO_ERR_HIP.  A result of another handle, a result that is no edge result, reserved != 0: PO_ERR_INVALID. */
po_status po_layout_merge(po_handle* h, po_result* edges, const po_merge_params* params, uint8_t* edge_flags_out,
                          po_result** merged_out);
po_status po_get_merge_stats(const po_handle* h, po_merge_stats* out);

/* The merged nodes of a po_layout_merge result: *n_paths = K and *n_members = the nodes on paths; then, up to the caps,
 * offsets_out[K + 1] (members of path k at [offsets[k], offsets[k + 1])), members_out (the path's nodes in order),
 * prefix_out (one per member: the weight of the link out of it, 0 for the last) and lengths_out[K] (the sum of the
 * prefixes plus the length of the last read).  Arrays are written only when the cap holds all of them (cap_paths >= K
 * for offsets and lengths, cap_members >= n_members for members and prefixes); any of them may be NULL.  On anything
 * but a merged graph: PO_ERR_INVALID. */
po_status po_result_merged_paths(po_result* merged, uint64_t* n_paths, uint64_t* n_members, uint64_t* offsets_out,
                                 uint64_t cap_paths, uint32_t* members_out, int32_t* prefix_out, uint64_t cap_members,
                                 int64_t* lengths_out);

/* ---------------------------------------------------------------------------------------------
 * The last computation of `phasm layout` before it writes the graph (phasm/cli/assembler.py:190-193):
 * average_coverage_path(g, read_alignments, [u, v]) (phasm/assembly_graph.py:544-591) for every edge.
 * --------------------------------------------------------------------------------------------- */

typedef struct {
    uint32_t reserved;           /* must be 0                                                                    */
} po_coverage_params;

typedef struct {
    uint64_t read_length_sum;    /* sum of len(r) over the distinct reads r aligning to a member of u or of v      */
    int64_t path_length;         /* weight + len(v)                                                              */
} po_edge_coverage;              /* 16 bytes; avg_coverage = read_length_sum / path_length                        */

typedef struct {
    uint64_t n_rows, n_edges;
    uint64_t n_nodes;            /* nodes with at least one edge                                                 */
    uint64_t n_pairs;            /* distinct (node, aligning read) pairs                                         */
    uint64_t max_set;            /* the largest per-node set                                                     */
    uint64_t n_zero_path;        /* edges with path_length == 0 (the reference raises ZeroDivisionError)         */
    uint64_t n_invalid;          /* edges or rows that name a read the handle does not hold (the call fails then) */
    float ms_sets, ms_edges, ms_total;
} po_coverage_stats;

/* `graph` is an edge result of this handle -- from po_layout_edges, po_layout_reduce, po_layout_tips, po_layout_diamonds
 * -- or a merged graph from po_layout_merge; `rows` is a row result of this handle (po_overlaps*, po_add_gfa,
 * po_result_from_rows; a host-only result is copied up).  Both stay valid and unchanged.  With
 *   A(x) = { b : some row (x, b, ...) } + { a : some row (a, x, ...) } over ALL rows -- those the filters of stage 1
 *          drop and those of contained reads included (alignment_recorder, assembler.py:65-76, sees every line);
 *          duplicates count once, a row present on one strand only counts as given, a row (x, x) puts x into A(x),
 *          x+ and x- are different elements;
 *   members of a node = the node itself, or the reads of the path of a merged node;
 * the entry of edge (u, v, weight, overlap_len), in the graph's edge order, is
 *   read_length_sum = the sum of len(r) over the union of A(m), m a member of u or of v;  path_length = weight + len(v)
 * (len of a merged node: its merged length), both exact 64-bit integers: the IEEE double quotient of the two equals the
 * reference's `read_length_sum / path_length` bit for bit.  A self-loop (U, U) takes U's members once.  A v of length 0
 * adds neither its length nor its aligning reads (the reference tests `bool(last)`).  An edge with path_length == 0 is
 * reported as it is and counted in n_zero_path.  Device memory beyond the inputs is linear: 40 bytes per row, 28 per
 * node, 16 per edge.  params may be NULL.  A graph without edges: PO_OK, nothing written.  There is no CPU fallback:
 * without a GPU the call returns PO_ERR_HIP.  A result of another handle, the wrong kind of result in either position,
 * reserved != 0, coverage_out NULL with edges present: PO_ERR_INVALID. */
po_status po_layout_coverage(po_handle* h, po_result* graph, po_result* rows, const po_coverage_params* params,
                             po_edge_coverage* coverage_out /* host, po_result_count(graph) entries */);
po_status po_get_coverage_stats(const po_handle* h, po_coverage_stats* out);

/* ---------------------------------------------------------------------------------------------
 * The first step of `phasm chain` (phasm/cli/assembler.py:289-304): the weakly connected components of the graph,
 * numbered as networkx.weakly_connected_components yields them.
 * --------------------------------------------------------------------------------------------- */

typedef struct {
    uint32_t reserved;           /* must be 0                                                                    */
} po_components_params;

typedef struct {
    uint32_t first_node;         /* the component's lowest-ranked node                                           */
    uint32_t n_nodes;
    uint64_t n_edges;            /* "Connected component %d with %d nodes and %d edges."                         */
} po_component;                  /* 16 bytes                                                                     */

typedef struct {
    uint64_t n_nodes;            /* nodes of the graph (those in its node order)                                 */
    uint64_t n_edges;
    uint64_t n_components;
    uint64_t n_singletons;       /* components of one node                                                       */
    uint64_t max_component_nodes, max_component_edges;
    uint64_t n_invalid;          /* edges with an end that is not in the node order (the call fails then)        */
    uint32_t n_rounds;           /* hook + jump rounds run, the one that changed nothing included                */
    uint32_t n_batches;          /* readbacks of the round loop                                                  */
    float ms_rounds, ms_label, ms_total;
} po_components_stats;

/* `graph` is a graph result of this handle: an edge result (po_layout_edges, po_layout_reduce, po_layout_tips,
 * po_layout_diamonds), a merged graph (po_layout_merge) or a po_graph_from_edges result; it stays valid and unchanged.
 * With the node order of po_result_node_order (n_order nodes; the rank of a node is its place in it): two nodes are in
 * one component iff a chain of edges joins them, direction ignored; a node without an edge is a component of its own; a
 * self-loop joins nothing.  Component i is the i-th in the order of each component's lowest-ranked node -- what
 * `for v in G: if v not in seen: yield bfs(v)` yields.  node_component_out: the component of every node, parallel to the
 * node order.  edge_component_out: the component of u of every edge, in the graph's edge order.  components_out: one
 * entry per component (room for n_order entries).  Any of the three may be NULL; *n_components_out is always written.
 * Only integers are involved: every output is the same on every run.  An edge with an end that is not in the node order
 * is counted in n_invalid; the call then fails with PO_ERR_INVALID and writes nothing.  Device memory beyond the inputs
 * is linear: at most 57 bytes per node (12 of them per slot of the sort, padded to a power of two) and 12 per edge.
 * params may be NULL.  An empty graph with an empty order: PO_OK, 0 components.  The rounds are bounded by n_order + 2
 * on the host; reaching the bound is PO_ERR_HIP with a message, never a partition.  There is no CPU fallback: without a
 * GPU the call returns PO_ERR_HIP.  A row result, a result of another handle, reserved != 0, n_components_out NULL:
 * PO_ERR_INVALID. */
po_status po_layout_components(po_handle* h, po_result* graph, const po_components_params* params,
                               uint32_t* node_component_out, uint32_t* edge_component_out, po_component* components_out,
                               uint64_t* n_components_out);
po_status po_get_components_stats(const po_handle* h, po_components_stats* out);

/* ---------------------------------------------------------------------------------------------
 * The first step of superbubble detection inside `phasm chain` (partition_graph, phasm/bubbles.py:32-84): the strongly
 * connected components of the graph and what the reference's partitions are made of.
 * --------------------------------------------------------------------------------------------- */

typedef struct {
    uint32_t reserved;           /* must be 0                                                                    */
} po_partition_params;

typedef struct {
    uint32_t first_node;         /* the SCC's lowest-ranked node                                                 */
    uint32_t n_nodes;
    uint64_t n_edges;            /* edges with both ends in the SCC, self-loops included                         */
    uint32_t n_r_in;             /* members with PO_PART_R_IN                                                    */
    uint32_t n_re_out;           /* members with PO_PART_RE_OUT                                                  */
} po_scc;                        /* 24 bytes                                                                     */

/* node_flags_out, one byte per node of the order */
#define PO_PART_R_IN 1u          /* an in-edge from outside the node's partition: the reference adds ('r_', v)   */
#define PO_PART_RE_OUT 2u        /* an out-edge to outside the node's partition: the reference adds (u, 're_')   */
#define PO_PART_START 4u         /* a singleton with in-degree 0 in the graph (a self-loop is an in-edge)        */
#define PO_PART_SINK 8u          /* a singleton with out-degree 0 in the graph                                   */

typedef struct {
    uint64_t n_nodes;            /* nodes of the graph (those in its node order)                                 */
    uint64_t n_edges;
    uint64_t n_sccs, n_nonsingleton_sccs, n_singletons;
    uint64_t n_self_loops;       /* edges (u, u)                                                                 */
    uint64_t max_scc_nodes, max_scc_edges;
    uint64_t n_trimmed;          /* nodes retired by the trim rounds                                             */
    uint64_t n_class[5];         /* edges per class byte                                                         */
    uint64_t n_invalid;          /* edges with an end that is not in the node order (the call fails then)        */
    uint32_t n_outer;            /* trim + colour iterations                                                     */
    uint32_t n_trim_rounds, n_forward_rounds, n_backward_rounds;   /* each phase's closing round included          */
    uint32_t n_batches;          /* readbacks of the round loops                                                 */
    float ms_ranks, ms_rounds, ms_label, ms_total;
} po_partition_stats;

/* `graph` is a graph result of this handle, of the kinds po_layout_components takes; it stays valid and unchanged.  With
 * the node order of po_result_node_order (n_order nodes; the rank of a node is its place in it): two nodes are in one SCC
 * iff each reaches the other along directed edges; a node without edges is an SCC of its own; a node is a SINGLETON iff
 * its SCC has one node, self-loop or not.  SCC i is the i-th in the order of each SCC's lowest-ranked node (networkx
 * yields SCCs in a DFS order, which is not reproduced).  The reference's partitions are: every non-singleton SCC, and
 * per weakly connected component all its singletons together (the acyclic partition).
 *   node_scc_out    the SCC of every node, parallel to the node order
 *   node_flags_out  PO_PART_* bits of every node, parallel to the node order
 *   edge_class_out  per edge, in the graph's edge order: 0 both ends in one non-singleton SCC; 1 both ends singletons (a
 *                   self-loop on a singleton included): an edge of the acyclic partition; 2 singleton -> member of a
 *                   non-singleton SCC; 3 member of a non-singleton SCC -> singleton; 4 between two non-singleton SCCs
 *   sccs_out        one entry per SCC (room for n_order entries)
 * Any of the four may be NULL; *n_sccs_out is always written.  Only integers are involved: every output is the same on
 * every run (the round counts of the stats are statistics).  An edge with an end that is not in the node order is
 * counted in n_invalid; the call then fails with PO_ERR_INVALID and writes nothing.  Device memory beyond the inputs is
 * linear: at most 78 bytes per node (12 of them per slot of the sort, padded to a power of two) and 9 per edge.  params
 * may be NULL.  An empty graph with an empty order: PO_OK, 0 SCCs.  Every round loop is bounded on the host (a phase by
 * its live nodes + 2, the iterations by n_order); reaching a bound is PO_ERR_HIP with a message, never a partition.
 * There is no CPU fallback: without a GPU the call returns PO_ERR_HIP.  A row result, a result of another handle,
 * reserved != 0, n_sccs_out NULL: PO_ERR_INVALID. */
po_status po_layout_partition(po_handle* h, po_result* graph, const po_partition_params* params, uint32_t* node_scc_out,
                              uint8_t* node_flags_out, uint8_t* edge_class_out, po_scc* sccs_out, uint64_t* n_sccs_out);
po_status po_get_partition_stats(const po_handle* h, po_partition_stats* out);

/* ---------------------------------------------------------------------------------------------
 * The second step of superbubble detection inside `phasm chain`: the superbubbles of the acyclic partitions
 * (SuperBubbleFinderDAG, phasm/bubbles.py:174-381, as find_superbubbles calls it on every acyclic partition,
 * bubbles.py:411-414).
 * --------------------------------------------------------------------------------------------- */

typedef struct {
    uint32_t reserved;           /* must be 0                                                                    */
} po_superbubble_params;

#define PO_NO_NODE 0xFFFFFFFFu   /* "no such node" in node_exit_out / node_inside_out                            */

typedef struct {
    uint32_t entrance, exit;     /* node ids                                                                     */
    uint32_t n_inside;           /* nodes strictly inside (neither end), those of nested superbubbles included   */
    uint32_t nested;             /* 1: another superbubble holds both ends                                       */
} po_superbubble;                /* 16 bytes                                                                     */

/* node_flags_out, one byte per node of the order */
#define PO_SB_ENTRANCE 1u        /* the node enters a superbubble (node_exit_out names its exit)                 */
#define PO_SB_EXIT 2u            /* the node exits a superbubble                                                 */
#define PO_SB_NESTED 4u          /* on the entrance: the superbubble is nested                                   */
#define PO_SB_SELF_LOOP 8u       /* a singleton with an edge (u, u): in no superbubble                           */

typedef struct {
    uint64_t n_nodes;            /* nodes of the graph (those in its node order)                                 */
    uint64_t n_edges;
    uint64_t n_p_nodes;          /* nodes of P: the singletons, 'r_' and 're_' where an edge reaches them         */
    uint64_t n_p_edges;          /* edges of P: class 1, ('r_', v) and (u, 're_')                                */
    uint64_t n_bubbles, n_nested;
    uint64_t n_self_loop_nodes;  /* singletons with an edge (u, u)                                               */
    uint64_t n_discarded;        /* pairs that are superbubbles but for a self-loop in them                      */
    uint64_t n_invalid;          /* edges with an end that is not in the node order (the call fails then)        */
    uint32_t n_levels_forward, n_levels_backward;   /* nodes on the longest path of P from a source / to a sink   */
    uint32_t n_scc_rounds;       /* rounds of the SCC stage (trim + forward + backward)                          */
    uint32_t n_level_rounds, n_discard_rounds;      /* each loop's closing round included                         */
    uint32_t n_batches;          /* readbacks of all round loops                                                 */
    float ms_partition, ms_levels, ms_dominators, ms_label, ms_total;
} po_superbubble_stats;

/* `graph` is a graph result of this handle, of the kinds po_layout_partition takes; it stays valid and unchanged.  Ranks,
 * SCCs, singletons, edge classes and the PO_PART_* flags are those of po_layout_partition.  The PARTITION GRAPH P is the
 * union over all weakly connected components of what partition_graph yields last: the singletons, the class-1 edges, an
 * edge 'r_' -> v for every singleton with PO_PART_R_IN | PO_PART_START and an edge v -> 're_' for every singleton with
 * PO_PART_RE_OUT | PO_PART_SINK (one shared 'r_' / 're_' gives the same pairs of real nodes as one per component: 'r_' has
 * no in-edge and 're_' no out-edge, so neither lies inside a bubble of two real nodes).  A pair (s, t) of real nodes,
 * s != t, is a SUPERBUBBLE iff t is reachable from s; the set U of nodes reachable from s without passing t equals the set
 * of nodes that reach t without passing s; P[U] is acyclic (a self-loop on any member of U, s and t included, is a cycle);
 * and no t' in U without t satisfies the three with s.  It is NESTED iff another superbubble's U holds both its ends.  A node
 * enters at most one superbubble and exits at most one.
 *   node_exit_out    the exit of the superbubble the node enters, else PO_NO_NODE; parallel to the node order
 *   node_inside_out  the entrance of the innermost superbubble whose U holds the node strictly (neither end), else
 *                    PO_NO_NODE: superbubble_nodes(g, s, t) is {s, t} plus the nodes whose chain of node_inside reaches s
 *   node_flags_out   PO_SB_* bits of every node
 *   bubbles_out      one entry per superbubble, in the order of the entrances' ranks (room for n_order entries)
 * Any of the four may be NULL; *n_bubbles_out is always written.  The cyclic partitions are not covered here
 * (po_layout_superbubbles_all covers them); the order in which the reference's finder yields the pairs is not reproduced; where an acyclic partition holds a
 * self-loop or lacks 'r_' or 're_' the definition above applies, not the finder's behaviour.  Only integers are involved:
 * every output is the same on every run (the round counts of the stats are statistics).  An edge with an end that is not
 * in the node order is counted in n_invalid; the call then fails with PO_ERR_INVALID and writes nothing.  Device memory
 * beyond the inputs is linear: at most 168 bytes per node (78 of them po_layout_partition's, whose workspaces the call
 * fills first; 90 its own) and 17 per edge (9 + 8).  params may be NULL.  An empty graph with an empty order: PO_OK, 0
 * superbubbles.  Every round loop is bounded on the host (by its live nodes + 2), the launches per level by the number of
 * singletons, the one walk along a tree path inside a kernel by twice its level; reaching a bound is PO_ERR_HIP with a
 * message, never a result.  There is no CPU fallback: without a GPU the call returns PO_ERR_HIP.  A row result, a result
 * of another handle, reserved != 0, n_bubbles_out NULL: PO_ERR_INVALID. */
po_status po_layout_superbubbles(po_handle* h, po_result* graph, const po_superbubble_params* params, uint32_t* node_exit_out,
                                 uint32_t* node_inside_out, uint8_t* node_flags_out, po_superbubble* bubbles_out,
                                 uint64_t* n_bubbles_out);
po_status po_get_superbubble_stats(const po_handle* h, po_superbubble_stats* out);

/* ---------------------------------------------------------------------------------------------
 * The superbubbles of the WHOLE graph, the cyclic partitions included: what find_superbubbles (phasm/bubbles.py:397-445)
 * reaches through graph_to_dag (bubbles.py:104-171) on every non-singleton SCC, plus the acyclic partitions, in one call.
 * --------------------------------------------------------------------------------------------- */

typedef struct {
    uint32_t reserved;           /* must be 0                                                                    */
} po_superbubble_all_params;

typedef struct {
    uint64_t n_nodes;            /* nodes of the graph (those in its node order)                                 */
    uint64_t n_edges;
    uint64_t n_invalid;          /* edges with an end that is not in the node order (the call fails then)        */
    uint64_t n_bubbles, n_nested;
    uint64_t n_cyclic_bubbles;   /* superbubbles whose entrance lies in a non-singleton SCC                       */
    uint64_t n_split;            /* nodes split in two, the largest number of any run                            */
    uint64_t n_rootless;         /* non-singleton SCCs without an edge from or to the outside (whole components) */
    uint64_t n_certified;        /* rootless SCCs whose runs ended with a root that lies on every cycle          */
    uint64_t n_edge_filtered;    /* pairs dropped because the graph has the edge exit -> entrance                */
    uint32_t n_split_levels;     /* SCC stages that split a node, the largest number of any run                  */
    uint32_t n_root_runs;        /* runs of the whole scheme: 1 unless a rootless SCC needs more roots           */
    uint32_t n_scc_rounds;       /* rounds of all SCC stages                                                     */
    uint32_t n_batches;          /* readbacks of all round loops                                                 */
    float ms_ranks, ms_split, ms_bubbles, ms_merge, ms_total;   /* the three in the middle: summed over the runs  */
} po_superbubble_all_stats;

/* `graph` is a graph result of this handle, of the kinds po_layout_partition takes; it stays valid and unchanged.  A pair
 * (s, t) of nodes, s != t, is a SUPERBUBBLE iff (1) t is reachable from s; (2) the set U of nodes reachable from s without
 * passing t equals the set of nodes that reach t without passing s; (3) G[U] is acyclic (a self-loop on any member of U is
 * a cycle, and so is an edge t -> s); (4) no other t' in U satisfies (1)-(3) with s.  This is the definition of
 * po_layout_superbubbles applied to the graph itself instead of to its acyclic partition; by the partition theorem of Sung
 * et al. it is the union of the same definition over everything partition_graph yields (each non-singleton SCC closed by
 * 'r_' / 're_', then the singletons).  So on the nodes whose SCC is a singleton the four outputs say exactly what
 * po_layout_superbubbles says (PO_SB_SELF_LOOP is set on every node with an edge (u, u) here, singleton or not).
 * The outputs, the NULL rules, PO_NO_NODE, the PO_SB_* bits, NESTED and n_inside are those of po_layout_superbubbles.
 * Not reproduced: the order in which the reference yields the pairs, its random.choice of a DFS root in an SCC without
 * 'r_', and its behaviour where its finder raises.
 * The scheme is ROOT SPLITTING: a node is split into a source that keeps its out-edges and a sink
 * that takes all its in-edges; per level one node of every SCC that is left, until none is; the stage of
 * po_layout_superbubbles runs on that graph of n_order + n_split ranks.  An SCC that is a whole weakly connected
 * component (n_rootless) is run once more per node of one shortest cycle through its lowest-ranked node, up to the first
 * node that lies on every cycle: n_root_runs is 1 + the largest number of such extra runs, at worst the length of that
 * cycle.  Only integers are involved: every output is the same on every run (round counts and batches are statistics).
 * An edge with an end that is not in the node order is counted in n_invalid; the call then fails with PO_ERR_INVALID and
 * writes nothing.  Device memory beyond the inputs is linear: at most 402 bytes per node (308: the workspaces of
 * po_layout_superbubbles, all but the sort and the node -> rank words twice, for the ranks of the flat graph; 94 its own)
 * and 25 per edge (17 + 8).  params may be NULL.  An empty graph with an empty order: PO_OK, 0 superbubbles.  Every loop is bounded on the
 * host: the round loops as in po_layout_superbubbles, the split levels by n_order + 2, the runs by the cycle's length;
 * reaching a bound is PO_ERR_HIP with a message, never a result.  There is no CPU fallback: without a GPU the call returns
 * PO_ERR_HIP.  A row result, a result of another handle, reserved != 0, n_bubbles_out NULL: PO_ERR_INVALID.
 * po_layout_bubblechains_all and po_layout_contigs_all build on this call's stage; po_layout_bubblechains, po_layout_contigs
 * and po_phase_paths still work on the acyclic partitions only. */
po_status po_layout_superbubbles_all(po_handle* h, po_result* graph, const po_superbubble_all_params* params, uint32_t* node_exit_out,
                                     uint32_t* node_inside_out, uint8_t* node_flags_out, po_superbubble* bubbles_out,
                                     uint64_t* n_bubbles_out);
po_status po_get_superbubble_all_stats(const po_handle* h, po_superbubble_all_stats* out);

/* ---------------------------------------------------------------------------------------------
 * The bubble chains of `phasm chain`: build_bubblechains (phasm/assembly_graph.py:594-652), as cli/assembler.py:272
 * calls it on every weakly connected component.
 * --------------------------------------------------------------------------------------------- */

typedef struct {
    uint32_t min_nodes;          /* a chain with fewer nodes is not reported (the reference's default: 1); 0 is invalid */
    uint32_t reserved;           /* must be 0                                                                    */
} po_bubblechain_params;

typedef struct {
    uint32_t first_entrance;     /* the head: the entrance of the chain's first bubble (node id)                 */
    uint32_t last_exit;          /* the exit of the chain's last bubble (node id)                                */
    uint32_t n_bubbles;          /* top-level bubbles of the chain                                               */
    uint32_t n_nodes;            /* nodes of the chain                                                           */
    uint64_t n_edges;            /* edges of the graph with both ends in the chain                               */
} po_bubblechain;                /* 24 bytes                                                                     */

typedef struct {
    uint64_t n_nodes;            /* nodes of the graph (those in its node order)                                 */
    uint64_t n_edges;
    uint64_t n_bubbles;          /* superbubbles of the acyclic partitions, nested ones included                 */
    uint64_t n_top;              /* ... of them not nested                                                       */
    uint64_t n_chains;           /* chains reported                                                              */
    uint64_t n_short;            /* chains dropped by min_nodes                                                  */
    uint64_t n_chain_nodes, n_chain_edges;   /* nodes / edges of the graph in a reported chain                   */
    uint64_t n_invalid;          /* edges with an end that is not in the node order (the call fails then)        */
    uint32_t max_chain_bubbles;  /* bubbles of the longest chain, dropped chains included                        */
    uint32_t n_nest_rounds, n_chain_rounds;  /* pointer-jumping rounds, each loop's closing round included       */
    uint32_t n_batches;          /* readbacks of all round loops, those of the superbubble stage included        */
    float ms_superbubbles, ms_chains, ms_label, ms_total;
} po_bubblechain_stats;

/* `graph` is a graph result of this handle, of the kinds po_layout_superbubbles takes; it stays valid and unchanged.  Ranks,
 * superbubbles, `nested` and the node_inside chains are exactly those of po_layout_superbubbles.  A TOP-LEVEL bubble is a
 * table entry with nested == 0: what find_superbubbles(g, report_nested=False) reports on an acyclic partition.  Bubble
 * (s, t) is LINKED to bubble (t, w) when both are top-level; a BUBBLE CHAIN is a maximal sequence of linked top-level
 * bubbles, its HEAD the entrance that is no top-level exit.  The links are acyclic (the structure graph is a DAG) and a node
 * enters at most one bubble and exits at most one, so chains are disjoint and every node lies in at most one.  The NODES of
 * a chain are the ends of its bubbles plus every node whose chain of node_inside reaches one of its entrances (nested
 * bubbles form no chain of their own: their nodes belong to the chain of the top-level bubble around them); its EDGES are
 * the graph's edges with both ends in the chain (the reference's networkx.subgraph).  A chain with fewer than min_nodes
 * nodes is not reported and its nodes carry no chain.  Chains are numbered by the rank of their heads.
 *   node_chain_out   the chain of the node, else PO_NO_NODE; parallel to the node order
 *   node_bubble_out  the 0-based position in its chain of the top-level bubble that holds the node, else PO_NO_NODE: for an
 *                    entrance the bubble it enters, for a chain's last exit the bubble it exits, for every other node the
 *                    bubble that holds it strictly
 *   edge_chain_out   in the graph's edge order: the chain when both ends carry the same one, else PO_NO_NODE
 *   chains_out       one entry per chain, in chain order (room for n_order entries)
 * Any of the four may be NULL; *n_chains_out is always written.  Not reproduced: the reference's numbering j, which follows
 * the iteration order of a Python set of node objects; cyclic partitions (graph_to_dag), as in po_layout_superbubbles; where
 * a component holds a non-singleton SCC or a self-loop the definition above applies, not the reference.  On a component
 * in which every SCC is a singleton and no node has a self-loop the reference yields exactly these chains (DESIGN.md
 * section 3.9k has the proof).  Only integers are involved: every output is the same on every run (the round counts of the
 * stats are statistics).  An edge with an end that is not in the node order is counted in n_invalid; the call then fails
 * with PO_ERR_INVALID and writes nothing.  Device memory beyond the inputs is linear: at most 260 bytes per node (168 of
 * them po_layout_superbubbles', whose workspaces the call fills first; 92 its own) and 21 per edge (17 + 4).  params may
 * be NULL (min_nodes 1).  An empty graph with an empty order: PO_OK, 0 chains.  Every round loop is bounded on the host (the
 * pointer jumping by its live entries + 2 rounds, though it needs only logarithmically many; the rest as in
 * po_layout_superbubbles); reaching a bound is PO_ERR_HIP with a message, never a result.  There is no CPU fallback: without
 * a GPU the call returns PO_ERR_HIP.  A row result, a result of another handle, reserved != 0, min_nodes == 0, n_chains_out
 * NULL: PO_ERR_INVALID. */
po_status po_layout_bubblechains(po_handle* h, po_result* graph, const po_bubblechain_params* params, uint32_t* node_chain_out,
                                 uint32_t* node_bubble_out, uint32_t* edge_chain_out, po_bubblechain* chains_out,
                                 uint64_t* n_chains_out);
po_status po_get_bubblechain_stats(const po_handle* h, po_bubblechain_stats* out);

/* ---------------------------------------------------------------------------------------------
 * The bubble chains of the WHOLE graph, the cyclic partitions included: po_layout_bubblechains behind the stage of
 * po_layout_superbubbles_all instead of po_layout_superbubbles.  A weak component that is one cycle (a circular chromosome,
 * a plasmid) becomes a RING CHAIN.
 * --------------------------------------------------------------------------------------------- */

typedef struct {
    uint64_t n_nodes;            /* the fields of po_bubblechain_stats, with the same meaning ...                */
    uint64_t n_edges;
    uint64_t n_bubbles;          /* superbubbles of the whole graph, nested ones included                        */
    uint64_t n_top;
    uint64_t n_chains;
    uint64_t n_short;
    uint64_t n_chain_nodes, n_chain_edges;
    uint64_t n_invalid;
    uint64_t n_ring_chains;      /* ... and: ring chains found, those that min_nodes dropped included            */
    uint64_t n_ring_bubbles;     /* top-level bubbles on them                                                    */
    uint64_t n_cyclic_bubbles;   /* as po_superbubble_all_stats; 0: the election of the ring leaders did not run */
    uint32_t max_chain_bubbles;
    uint32_t n_nest_rounds, n_chain_rounds;
    uint32_t n_batches;
    uint32_t n_ring_rounds;      /* rounds of the election: ceil(log2(n_top)) + 1 where it ran, else 0           */
    uint32_t n_root_runs, n_split_levels;   /* of the first stage, as po_superbubble_all_stats                   */
    uint32_t reserved;
    float ms_superbubbles, ms_chains, ms_label, ms_total;
} po_bubblechain_all_stats;

/* `graph` is a graph result of this handle, of the kinds po_layout_superbubbles_all takes; it stays valid and unchanged.
 * Ranks, superbubbles, `nested` and the node_inside chains are exactly those of po_layout_superbubbles_all.  TOP-LEVEL
 * bubbles, LINKS, the NODES and EDGES of a chain, the min_nodes filter, the four outputs, their NULL rules and PO_NO_NODE are
 * those of po_layout_bubblechains.  A node still enters at most one top-level bubble and exits at most one, but inside an
 * SCC the links need not be acyclic: they form disjoint paths and RINGS, (s0, s1) -> (s1, s2) -> ... -> (sk-1, s0).  A
 * path is a chain as before, its HEAD the entrance that is no top-level exit.  A RING CHAIN holds ALL the bubbles of its
 * ring; its head is the entrance with the lowest rank on the ring, the positions count the bubbles from there along the
 * links, and
 *   last_exit == first_entrance     (this equality marks a ring chain: on a path chain the two differ)
 *   n_bubbles                       all bubbles of the ring
 *   node_bubble_out of the head     0, the bubble it enters (it is also the exit of the last bubble)
 * Chains, rings among them, are numbered by the rank of their heads.  On a graph in which every SCC is a singleton the
 * outputs are byte-equal to po_layout_bubblechains'.
 * Not reproduced, beyond what po_layout_bubblechains and po_layout_superbubbles_all list: on a ring the reference's
 * build_bubblechains starts its walk at an arbitrary entrance (the iteration order of a Python set) and stops ONE BUBBLE
 * SHORT, because at the closing bubble both ends are already visited; its node set is this call's minus the strict
 * interior of exactly one top-level bubble of the ring (DESIGN.md section 3.9u has the evidence).
 * The ring leaders are elected by a fixed number of pointer-doubling rounds, ceil(log2(n_top)) + 1, without a readback;
 * the election runs only when the first stage reported n_cyclic_bubbles > 0.  Only integers are involved: every output is
 * the same on every run.  An edge with an end that is not in the node order is counted in n_invalid; the call then fails
 * with PO_ERR_INVALID and writes nothing.  Device memory beyond the inputs is linear: at most 510 bytes per node (402 of them
 * po_layout_superbubbles_all's, whose workspaces the call fills first; 92 those of po_layout_bubblechains; 16 the two buffer
 * pairs of the election) and 29 per edge (25 + 4).  params may be NULL (min_nodes 1).  An empty graph with an empty order:
 * PO_OK, 0 chains.  Every loop is bounded on the host as in po_layout_superbubbles_all and po_layout_bubblechains, the
 * election by its fixed count; heads and ring leaders that do not add up, or a node whose ranking reached no head, are
 * PO_ERR_HIP with a message, never a result.  There is no CPU fallback: without a GPU the call returns PO_ERR_HIP.  A row
 * result, a result of another handle, reserved != 0, min_nodes == 0, n_chains_out NULL: PO_ERR_INVALID.
 * po_phase_paths, and with it `phasm phase` and the walk, still take the acyclic partitions only. */
po_status po_layout_bubblechains_all(po_handle* h, po_result* graph, const po_bubblechain_params* params, uint32_t* node_chain_out,
                                     uint32_t* node_bubble_out, uint32_t* edge_chain_out, po_bubblechain* chains_out,
                                     uint64_t* n_chains_out);
po_status po_get_bubblechain_all_stats(const po_handle* h, po_bubblechain_all_stats* out);

/* ---------------------------------------------------------------------------------------------
 * The contigs of `phasm chain` outside the bubble chains: identify_contigs (phasm/assembly_graph.py:655-718), as
 * cli/assembler.py:289 calls it on every weakly connected component behind build_bubblechains.
 * --------------------------------------------------------------------------------------------- */

typedef struct {
    uint64_t min_contig_len;     /* a shorter path or node is not reported (the reference's default: 5000); 0 is valid  */
    uint32_t min_nodes;          /* of the bubble chains whose nodes are excluded, as po_bubblechain_params; 0 is invalid */
    uint32_t reserved;           /* must be 0                                                                    */
} po_contig_params;

typedef struct {
    uint32_t first_node;         /* the first node of the path (node id)                                         */
    uint32_t last_node;          /* its last node; the first again on a path that ends where it began            */
    uint32_t n_nodes;            /* nodes on the path, counted as often as they occur; 1 for a one-node contig   */
    uint32_t first_edge;         /* the head edge, as an index in the graph's edge order; PO_NO_NODE for a one-node contig */
    int64_t length;              /* sum of the weights of the path's edges + the length of the last node         */
} po_contig;                     /* 24 bytes                                                                     */

typedef struct {
    uint64_t n_nodes;            /* nodes of the graph (those in its node order)                                 */
    uint64_t n_edges;
    uint64_t n_invalid;          /* edges with an end that is not in the node order (the call fails then)        */
    uint64_t n_excluded;         /* nodes in the exclude set                                                     */
    uint64_t n_root_starts;      /* edges (a, b) with in(a) != 1                                                 */
    uint64_t n_late_starts;      /* edges (a, b) with in(a) == 1 and out(a) > 1                                  */
    uint64_t n_blocked;          /* starts with both ends excluded                                               */
    uint64_t n_covered_edges, n_uncovered_edges;   /* their sum is n_edges                                       */
    uint64_t n_paths;            /* covered starts: each is the head edge of one path                            */
    uint64_t n_short_paths;      /* ... of them dropped by min_contig_len                                        */
    uint64_t n_isolated;         /* nodes without an edge                                                        */
    uint64_t n_short_isolated;   /* ... of them dropped by min_contig_len                                        */
    uint64_t n_contigs;          /* n_paths - n_short_paths + n_isolated - n_short_isolated                      */
    uint64_t max_path_nodes;     /* nodes of the longest path, dropped ones included                             */
    uint64_t n_chains;           /* bubble chains whose nodes were excluded (0 with exclude_in)                  */
    uint32_t n_path_rounds, n_cover_rounds;   /* pointer-jumping rounds, each loop's closing round included      */
    uint32_t n_batches;          /* readbacks of all round loops, those of the stages run first included         */
    uint32_t reserved;
    float ms_ranks, ms_bubblechains, ms_paths, ms_cover, ms_label, ms_total;
} po_contig_stats;

/* `graph` is a graph result of this handle, of the kinds po_layout_bubblechains takes; it stays valid and unchanged.  With
 * in(x) / out(x) the degrees in the graph and X the excluded nodes, an edge (a, b) is a ROOT START when in(a) != 1, a LATE
 * START when in(a) == 1 and out(a) > 1, an EXTENSION when in(a) == 1 and out(a) == 1; a start is BLOCKED when a and b are
 * both in X.  COVERED is the least fixed point of: a root start is covered iff it is not blocked; a late start (a, .) iff the
 * one in-edge of a is covered and the start is not blocked; an extension (a, .) iff the one in-edge of a is covered.  Rings
 * of in-degree-1 nodes, and what hangs off them through in-degree-1 nodes, are never covered.  Every covered start (a, b) is
 * the HEAD EDGE of one path [a, b, c, ...]: from cur = b the path takes the one out-edge of cur while out(cur) == 1 and
 * in(cur) == 1 (extensions never look at X: a path that starts outside X runs on through it).  Every covered edge lies on
 * exactly one path; a path may end at its own first node.  The LENGTH of a path is the signed 64-bit sum of the weights of
 * its edges plus the length of its last node (a read's from the handle, a merged node's from the graph); a path is reported
 * iff length >= min_contig_len, compared in 64 bits.  Every node without an edge whose length is >= min_contig_len is
 * reported as a one-node contig.  This is what the reference's queue walk reports, as a set of paths (DESIGN.md section
 * 3.9l has the argument).  Contigs are numbered: the reported paths by (rank of the head edge's first node, index of the
 * head edge in the edge order), then the one-node contigs by rank.
 *   exclude_in       NULL: the call runs po_layout_bubblechains' stages first, in their workspaces, and X = the nodes that
 *                    carry a chain after the min_nodes filter (what `phasm chain` passes).  Else one byte per node,
 *                    parallel to the node order, non-zero = in X; the bubble-chain stages are skipped, min_nodes is ignored
 *   edge_contig_out  in the graph's edge order: the contig whose path holds the edge, else PO_NO_NODE (uncovered, or the
 *                    path was dropped by its length)
 *   edge_pos_out     the 0-based place of the edge on that path (the head edge 0), else PO_NO_NODE
 *   contigs_out      one entry per contig, in contig order (room for n_order + n_edges entries)
 * Any of the three may be NULL; *n_contigs_out is always written.  The two edge arrays identify every path completely; a
 * node may end several paths, so there is no output per node.  Not reproduced: the reference's numbering j, the pop order
 * of a queue filled in the iteration order of a Python set.  Only integers are involved: every output is the same on every
 * run (the round counts of the stats are statistics).  An edge with an end that is not in the node order is counted in
 * n_invalid; the call then fails with PO_ERR_INVALID and writes nothing.  Device memory beyond the inputs and the rank
 * scaffold is linear: 49 bytes per node and at most 120 per edge of its own, plus with exclude_in == NULL what
 * po_layout_bubblechains takes.  params may be NULL (5000, 1).  An empty graph with an empty order: PO_OK, 0 contigs.  Both
 * pointer-jumping loops are bounded on the host (edges + 2 rounds, though they need ceil(log2(longest)) + 1); reaching a
 * bound is PO_ERR_HIP with a message, never a result.  There is no CPU fallback: without a GPU the call returns PO_ERR_HIP.
 * A row result, a result of another handle, reserved != 0, min_nodes == 0, n_contigs_out NULL: PO_ERR_INVALID. */
po_status po_layout_contigs(po_handle* h, po_result* graph, const po_contig_params* params, const uint8_t* exclude_in,
                            uint32_t* edge_contig_out, uint32_t* edge_pos_out, po_contig* contigs_out, uint64_t* n_contigs_out);
po_status po_get_contig_stats(const po_handle* h, po_contig_stats* out);

/* po_layout_contigs with the chains of po_layout_bubblechains_all: with exclude_in == NULL the call runs that call's stages
 * first and X = the nodes that carry one of ITS chains after the min_nodes filter, ring chains included, so no piece of a
 * circular component that is a ring chain is reported as a contig.  The definition of the contigs, the parameters, the
 * outputs, their NULL rules, the limits and the errors are those of po_layout_contigs; with exclude_in != NULL the two calls
 * do the same.  Device memory: as po_layout_contigs, with what po_layout_bubblechains_all takes in place of
 * po_layout_bubblechains.  The stats are those of po_get_contig_stats. */
po_status po_layout_contigs_all(po_handle* h, po_result* graph, const po_contig_params* params, const uint8_t* exclude_in,
                                uint32_t* edge_contig_out, uint32_t* edge_pos_out, po_contig* contigs_out, uint64_t* n_contigs_out);

/* ---------------------------------------------------------------------------------------------
 * The hot loop of `phasm phase`: BubbleChainPhaser.branch -- generate_new_hsets and calculate_rl, phasm/phasing.py:421-480,
 * 564-631 -- and prune (phasing.py:482-539) at ONE bubble, given as plain arrays.  The call needs neither reads nor a graph on
 * the handle.  Not part of it: the state the bubble walk of phase() carries, new_block and the final prune(.., 1.0) (po_walk_*
 * below), its random.choice among ties, spelling sequences (po_spell), CoverageModel (which the reference never uses), and the
 * superbubbles of cyclic partitions.
 * --------------------------------------------------------------------------------------------- */

typedef struct {
    uint32_t ploidy;             /* k, 1..8                                                                         */
    uint32_t n_paths;            /* P, 1..64: the possible paths through the bubble                                 */
    uint32_t n_cands;            /* C >= 1: the candidate haplotype sets                                            */
    uint32_t n_reads;            /* R >= 0: the relevant reads                                                      */
    uint32_t n_b;                /* local read ids are 0..n_b-1: the graph reads that are b read of an alignment    */
    uint32_t start_of_block;     /* non-zero: only the non-decreasing k-tuples (combinations_with_replacement)      */
    uint32_t min_spanning_reads; /* R below it: every rl is -inf                                                    */
    uint32_t prune;              /* non-zero: the kept list goes through prune before it comes out                  */
    uint32_t max_candidates;     /* prune: stop raising the level once this many or fewer survive                   */
    uint32_t n_levels;           /* prune: the number of levels in po_phase_input.levels, at most 1024              */
    double threshold;            /* linear, >= 0; 0 stands for log10 = -inf                                         */
    uint32_t reserved;           /* must be 0                                                                       */
    uint32_t reserved2;          /* must be 0                                                                       */
} po_phase_params;

typedef struct {
    const int32_t* overlap_max;  /* [n_reads]; may be <= 0 (the reference computes edge_length - la.arange[0])      */
    const uint32_t* aln_off;     /* [n_reads + 1]: the alignments of read r are aln_off[r] .. aln_off[r+1]-1        */
    const uint32_t* aln_b;       /* per alignment: local id of its b read                                           */
    const int32_t* aln_a0;       /* per alignment: arange[0]                                                        */
    const int32_t* aln_a1;       /* per alignment: arange[1]                                                        */
    const uint32_t* path_off;    /* [n_paths + 1]                                                                   */
    const uint32_t* path_ids;    /* per path the local ids of its interior reads (MergedReads expanded, entrance
                                    and exit left out)                                                              */
    const uint32_t* set_off;     /* [n_cands * ploidy + 1]: list c * ploidy + i is read_sets[i] of candidate c      */
    const uint32_t* set_ids;     /* the local ids of those reads (reads outside 0..n_b-1 can never match: the
                                    caller leaves them out)                                                         */
    const double* levels;        /* [n_levels]: log10 of the prune factors f0, f0 + step, ... in the order the
                                    reference's loop would reach them (it accumulates in float and stops at
                                    factor >= 1.0 or after max_prune_rounds rounds)                                 */
} po_phase_input;

typedef struct {
    uint64_t n_extensions;       /* extensions enumerated: C * P^k, at the start of a block C * (P+k-1 choose k)     */
    uint64_t n_kept;             /* of them with rl >= log10(threshold)                                             */
    uint64_t n_survivors;        /* what prune left of those (= n_kept without prune or at its early returns)       */
    uint64_t level_counts[16];   /* survivors of the first 16 levels, each as if the loop had got there             */
    double max_rl;               /* greatest rl of the kept list (NaN: the list is empty)                           */
    int32_t level_used;          /* index of the level prune stopped at; -1: it did not filter                      */
    uint32_t n_levels;
    float ms_intervals, ms_table, ms_extend, ms_filter, ms_prune, ms_total;
} po_phase_stats;

/* 1. TABLE.  For candidate c, haplotype slot i and path p, in float64,
 *      S[c][i][p] = sum over the relevant reads r of f(r; read_sets[i] of c + interior of p)
 *      f = (E - S0) / overlap_max_r if S0 < E, else 0
 *    where S0 is the least arange[0] and E the greatest min(overlap_max_r, arange[1]), never below 0, of the alignments of r
 *    whose b read is in the set (S0 < E fails when none is).  The sum runs in the implementation's order, which is fixed (per
 *    tile of 2048 reads: per thread in index order, lanes by a butterfly, waves in order; tiles in order): there are no
 *    floating-point atomics, the same input gives the same bits on every run.
 * 2. EXTENSIONS.  Not at the start of a block all P^k tuples (p_0 .. p_{k-1}) in itertools.product order; at the start of a
 *    block only the non-decreasing ones, in combinations_with_replacement order.  The ID of an extension is its product index
 *    in both modes: digits base P, slot 0 most significant.
 * 3. SCORE.  tot = (S[c][0][p_0] + ... + S[c][k-1][p_{k-1}]) / (k * R), added in slot order; p_sr = log10(tot), -inf when
 *    tot == 0 (and when R == 0); prior = log10(multinomial / P^k) with multinomial = k! / prod m_j! over the multiplicities m_j
 *    by path INDEX; rl = p_sr + prior.  R < min_spanning_reads: rl = -inf for every extension.
 * 4. FILTER.  An extension is kept iff rl >= log10(threshold) (threshold 0: -inf >= -inf keeps the all-zero ones, as in the
 *    reference).  The kept entries (cand, ext, rl) come out in (cand ascending, ext ascending) order -- the order of the list
 *    branch returns.  Compaction is by prefix sum, not by atomics.
 * 5. PRUNE (params.prune != 0): the reference's prune on the kept list with its early returns -- fewer than 2 entries, no
 *    levels (the caller passes none for a factor <= 0), greatest rl = -inf: the list comes out as it is.  Otherwise an entry
 *    survives level j iff rl - max >= levels[0..j] all hold; the call counts the survivors of every level in one pass, takes
 *    the first level j with count <= max_candidates, else the last, and the survivors of that level come out in the same
 *    order.  A level above 0 removes everything, as in the reference.
 * 6. OUTPUTS.  Up to `cap` entries are written to cand_out / ext_out / rl_out (each may be NULL); *n_out is always the full
 *    count (the convention of po_result_node_order).  table_out (may be NULL) receives S as C * k * P doubles; with C = 1 and
 *    empty sets S[0][0][p] / R is the score of phase_large_bubble (phasing.py:633-685).  po_get_phase_stats has the counts.
 * 7. REJECTIONS, each PO_ERR_INVALID with a sentence in po_last_error, checked on the host before the device is touched, the
 *    outputs untouched (*n_out = 0 where it is given): n_out NULL; params or input NULL; reserved != 0, a threshold that is
 *    negative or NaN, more than 1024 levels; ploidy outside 1..8; n_paths outside 1..64; n_cands == 0; C * P^k >= 2^31 (the id
 *    space, in both modes); a missing array; offsets that do not start at 0 or that decrease; a local id >= n_b.
 * Where the reference would raise (overlap_max == 0 under a negative arange[0]: ZeroDivisionError; a negative sum: log10
 * domain error; R == 0 with min_spanning_reads == 0) the call computes in IEEE arithmetic; a NaN rl is never kept.  Device
 * memory is linear in (C*k + P) * (R + n_b/8), C*k*P and C * P^k (13 bytes per extension id, 21 per kept entry, 16 per survivor).  There is no
 * CPU fallback: without a GPU a valid call returns PO_ERR_HIP. */
po_status po_phase_branch(po_handle* h, const po_phase_params* params, const po_phase_input* input, uint32_t* cand_out,
                          uint32_t* ext_out, double* rl_out, uint64_t cap, double* table_out, uint64_t* n_out);
po_status po_get_phase_stats(const po_handle* h, po_phase_stats* out);

/* ---------------------------------------------------------------------------------------------
 * The relevant reads of a bubble of `phasm phase`: the arrays po_phase_branch takes, from the rows.
 *   _get_read_alignments (phasm/cli/assembler.py:313-328), get_aligning_reads (phasm/phasing.py:541-550), the spanning-read
 *   intersection (phasing.py:263-286), get_relevant_read_info and _get_max_possible_overlap (phasing.py:366-419).
 * Not part of it: the bubble walk itself, new_block, the final random.choice (all_simple_paths, the interior and the exit
 * predecessors of every bubble: po_phase_paths; spelling: po_spell); the outputs of the
 * gather come to the host (they are bubble-sized), po_phase_branch takes them from there.
 * --------------------------------------------------------------------------------------------- */

typedef struct {
    uint32_t b;                  /* y: the oriented read the entry of (x, y) aligns x to                            */
    int32_t a0, a1;              /* arange of the winning write                                                     */
    uint32_t seq;                /* its sequence number: 2 * row for m[a][b], 2 * row + 1 for m[b][a]               */
} po_alignment;

typedef struct {
    uint64_t n_rows, n_keys, max_degree, n_invalid;
    float ms_insert, ms_fill, ms_place, ms_total;
} po_phase_index_stats;

/* THE INDEX: the reference's read_alignments mapping of a row result, on the device.  For every row
 * i = (a, b, astart, aend, bstart, bend), in row order, the reference writes m[a][b] = (astart, aend) -- sequence number 2i --
 * and then m[b][a] = (bstart, bend) -- 2i + 1; a later write replaces an earlier one, so the entry of key (x, y) is the write
 * with the greatest sequence number.  x+ and x- are different keys.  A later row (b, a, ..) therefore replaces what an
 * earlier (a, b, ..) wrote under both keys, and a row (x, x, ..) leaves (bstart, bend) under (x, x).
 * Form: CSR over the handle's oriented read ids (< po_num_sequences): per x the distinct y as po_alignment, ascending in y;
 * beside it the open-addressing table of the 64-bit keys (x, y) for point look-ups.  Two runs give the same bytes.
 * The result is of a kind of its own: it holds no rows (po_result_count is 0), it is freed with po_result_free, and it stays
 * valid after `rows` is freed.  It describes the reads the handle held when it was built: after more reads are added the
 * gather refuses it.
 * Limits: 2 * rows < 2^31, else PO_ERR_CAPACITY.  A row that names a read the handle does not hold: PO_ERR_INVALID (counted in
 * n_invalid).  Device memory of the index: at most 80 bytes per row + 8 per read; while it is built another 40 per row + 8 per
 * read in workspaces of the handle.  There is no CPU fallback. */
po_status po_phase_index(po_handle* h, po_result* rows, po_result** index_out);
/* For tests and tools: the offsets (n_ids + 1 of them, n_ids = po_num_sequences when the index was built) and up to `cap`
 * entries in ascending (x, y); *n_out is always the number of keys (the convention of po_result_node_order).  Either array
 * may be NULL. */
po_status po_phase_index_copy(po_result* index, uint64_t* off_out, po_alignment* entries_out, uint64_t cap, uint64_t* n_out);
po_status po_get_phase_index_stats(const po_handle* h, po_phase_index_stats* out);

typedef struct {
    uint32_t mode;               /* 0 = spanning (not the start of a block), 1 = all (the start of a block)         */
    uint32_t min_spanning_reads;
    uint32_t reserved, reserved2; /* must be 0                                                                      */
} po_relevant_params;

typedef struct {
    const uint32_t* cur_graph;     uint64_t n_cur_graph;     /* interior reads of the bubble, MergedReads expanded  */
    const uint32_t* prev_graph;    uint64_t n_prev_graph;    /* self.prev_graph_reads                               */
    const uint32_t* prev_aligning; uint64_t n_prev_aligning; /* self.prev_aligning_reads                            */
    /* the predecessors of the exit that are PLAIN reads, with g[pred][exit][edge_len].  A MergedReads predecessor is never
     * a key of the mapping (`pred in self.alignments` is false for it), so it contributes len(read), which is where the
     * minimum starts: the caller leaves it out. */
    const uint32_t* pred_read; const int32_t* pred_edge_len; uint64_t n_pred;
} po_relevant_input;

/* what po_relevant_sizes gives (C has one name space for types and functions, so the struct has a name of its own) */
typedef struct {
    uint64_t n_cur_aligning, n_spanning, n_relevant, n_alignments, n_b;
    uint32_t fell_back, reserved;
} po_relevant_dims;

typedef struct {
    uint64_t n_cur_aligning, n_spanning, n_relevant, n_alignments, n_b;
    uint32_t fell_back, reserved;
    float ms_mark, ms_lists, ms_alignments, ms_total;
} po_relevant_stats;

/* THE GATHER for one bubble.  All lists are oriented read ids; duplicates are allowed and count once.
 *   cur_aligning = cur_graph + { y : (x, y) in the index, x in cur_graph }, ascending.
 *   n_spanning   = |prev_aligning & cur_aligning|.
 *   The relevant reads: mode 1: cur_aligning.  Mode 0 with n_spanning >= min_spanning_reads: the intersection.  Mode 0 with
 *   n_spanning < min_spanning_reads: fell_back = 1 and the call computes what the reference computes after new_block()
 *   (phasing.py:266-286): cur_aligning, with prev_graph taken as empty.
 *   G = cur_graph + prev_graph (after the fallback rule); b_reads is G ascending, n_b = |G|, the local id of a read its place
 *   in b_reads.
 *   For relevant read r, in ascending order of id: its alignments are the entries (r, y) with y in G, as (local(y), a0, a1), in
 *   ascending y; overlap_max[r] = min(len(r), min over the given preds p with (p, r) in the index of pred_edge_len[p] -
 *   a0(p, r)), as int32; it may be <= 0.
 * overlap_max, aln_off, aln_b, aln_a0, aln_a1 are exactly those fields of po_phase_input.  The result is of a kind of its own,
 * freed with po_result_free; po_relevant_sizes gives the lengths (cur_aligning: n_cur_aligning; rel_reads, overlap_max:
 * n_relevant; aln_off: n_relevant + 1; aln_b, aln_a0, aln_a1: n_alignments; b_reads: n_b), po_relevant_copy the arrays, each
 * of which may be NULL.
 * Rejections, each PO_ERR_INVALID with a sentence in po_last_error, checked on the host before the device is touched (*out
 * stays NULL): NULL out, params or input; reserved != 0; mode > 1; a NULL list with a non-zero count; an id >=
 * po_num_sequences; a result of another handle or of the wrong kind; an index built before reads were added.  An empty
 * cur_graph is PO_OK with every size 0.  Work per call is proportional to the segments of cur_graph and of the relevant reads
 * plus n_ids / 32 words, not to the rows.  There is no CPU fallback: without a GPU a valid call returns PO_ERR_HIP. */
po_status po_phase_relevant(po_handle* h, po_result* index, const po_relevant_params* params, const po_relevant_input* input,
                            po_result** out);
po_status po_relevant_sizes(const po_result* out, po_relevant_dims* sizes);
po_status po_relevant_copy(po_result* out, uint32_t* cur_aligning, uint32_t* rel_reads, int32_t* overlap_max, uint32_t* aln_off,
                           uint32_t* aln_b, int32_t* aln_a0, int32_t* aln_a1, uint32_t* b_reads);
po_status po_get_relevant_stats(const po_handle* h, po_relevant_stats* out);

/* ---- SPELLING: the sequences of graph paths out of the reads the handle holds (phasm_amd/csrc/spell.hip.h) ----
 * What AssemblyGraph.sequence_for_path and SequenceSource.get_sequence of the reference return, once the caller has reduced
 * every path to PIECES: piece p = (piece_read[p], piece_take[p]) stands for the first piece_take[p] bytes of oriented read
 * piece_read[p] as it was added (po_add_sequence, po_add_fasta), 0 <= take <= the read's length.  Sequence s is the
 * concatenation of the pieces seq_off[s] .. seq_off[s + 1] - 1, with ASCII a-z as A-Z and every other byte unchanged.  The
 * arrays are host memory; seq_off has n_seqs + 1 entries, begins with 0, ascends and ends with n_pieces. */
typedef struct {
    uint64_t n_seqs, n_pieces;
    const uint64_t* seq_off;
    const uint32_t* piece_read;
    const uint32_t* piece_take;
} po_spell_input;

typedef struct {
    uint64_t n_seqs, n_pieces, n_bytes;
    uint64_t n_patched;   /* exception records of a 2-bit store that lay inside a piece */
    float device_ms;      /* upload of the pieces, scan, decode and patch; not the copy of the bytes to the host */
    uint32_t reserved;
} po_spell_stats;

/* po_spell uploads the reads first if the read set changed since the last upload; the bytes stay on the device with the
 * result, which is of a kind of its own and freed with po_result_free.  po_spell_sizes gives the number of sequences and of
 * bytes; po_spell_copy the n_seqs + 1 byte offsets of the sequences and the first min(cap, n_bytes) bytes, all sequences back
 * to back; either array may be NULL.  Zero sequences, zero pieces and sequences of zero bytes are valid.
 * Rejections, checked on the host before the device is touched (*out stays NULL): PO_ERR_INVALID for a NULL argument, a read
 * id >= po_num_sequences, a take greater than the read's length, a seq_off that does not begin with 0, ascend and end with
 * n_pieces, and a handle whose sequences were added by po_add_segment or po_add_gfa (lengths, no bases); PO_ERR_CAPACITY for
 * more than 2^32 - 16 bytes or 2^32 - 2 pieces in one call: the caller splits the call.  Offsets are 64-bit throughout.
 * There is no CPU fallback: without a GPU a valid call returns PO_ERR_HIP. */
po_status po_spell(po_handle* h, const po_spell_input* in, po_result** out);
po_status po_spell_sizes(const po_result* out, uint64_t* n_seqs, uint64_t* n_bytes);
po_status po_spell_copy(po_result* out, uint64_t* seq_byte_off, uint8_t* bytes, uint64_t cap);
po_status po_get_spell_stats(const po_handle* h, po_spell_stats* out);

/* ---------------------------------------------------------------------------------------------
 * What BubbleChainPhaser.phase() of `phasm phase` computes per bubble before it looks at a read (phasm/phasing.py:196-234, 396),
 * for every top-level bubble of a graph in one call (phasm_amd/csrc/paths.hip.h):
 *   the order of the bubbles along their chain; networkx.all_simple_paths(g, entrance, exit);
 *   superbubble_nodes(g, entrance, exit) - {entrance, exit}; the predecessors of the exit with g[p][exit]['weight'].
 * Not part of it: the walk loop itself, new_block, the final random.choice, the reads of a node (get_all_reads).
 * --------------------------------------------------------------------------------------------- */

typedef struct {
    uint64_t max_paths;          /* the paths of a bubble are listed iff n_paths <= max_paths; 0: counts only           */
    uint32_t reserved;           /* must be 0                                                                       */
} po_paths_params;

#define PO_PATHS_MANY 0xFFFFFFFFFFFFFFFFull   /* n_paths of a bubble with at least 2^64 - 1 paths                  */
#define PO_PATHS_BARE 1u         /* no interior node: non_branching_bubble drops the bubble, the walk of its chain ends */
#define PO_PATHS_UNLISTED 2u     /* more than max_paths paths: the count only                                       */
#define PO_PATHS_SATURATED 4u    /* the count hit PO_PATHS_MANY; implies PO_PATHS_UNLISTED                          */

typedef struct {
    uint32_t entrance, exit;     /* node ids                                                                        */
    uint32_t chain, position;    /* as po_layout_bubblechains with min_nodes = 1 numbers them                       */
    uint32_t n_inside;           /* interior nodes, those of nested bubbles included (n_inside of po_superbubble)   */
    uint32_t flags;              /* PO_PATHS_*                                                                      */
    uint64_t n_paths;            /* simple paths from entrance to exit, saturating at PO_PATHS_MANY                 */
    uint64_t n_path_nodes;       /* nodes of its listed paths together, both ends of each included; 0 when unlisted */
} po_bubble_paths;               /* 40 bytes                                                                        */

/* what po_paths_sizes gives */
typedef struct {
    uint64_t n_bubbles, n_inside_nodes, n_preds, n_listed_paths, n_path_nodes;
} po_paths_dims;

typedef struct {
    uint64_t n_nodes, n_edges;   /* of the graph (the nodes: those in its node order)                               */
    uint64_t n_invalid;          /* edges with an end that is not in the node order (the call fails then)           */
    uint64_t n_bubbles, n_bare, n_unlisted, n_saturated, n_listed_paths, n_path_nodes;
    uint64_t max_paths_seen;     /* the greatest n_paths of a bubble                                                */
    uint64_t max_path_nodes;     /* nodes of the longest listed path                                                */
    uint64_t n_stray_edges;      /* out-edges of a bubble member that leave U + {t}: 0 by the definition            */
    uint32_t n_count_rounds;     /* counting rounds, the closing round included                                     */
    uint32_t n_batches;          /* readbacks of all round loops, those of the stages before included               */
    float ms_chains, ms_count, ms_list, ms_total;
} po_paths_stats;

/* `graph` is a graph result of this handle, of the kinds po_layout_bubblechains takes; it stays valid and unchanged.
 * BUBBLES: every top-level superbubble of the acyclic partitions (the nested == 0 entries of po_layout_superbubbles: what
 * find_superbubbles(g, report_nested=False) reports), one table entry each, ordered by (chain, position) as
 * po_layout_bubblechains with min_nodes = 1 defines them: within a chain the order in which phase() visits them.  Nested
 * bubbles get no entry; their nodes are interior nodes of the top-level bubble around them.  Cyclic partitions stay out.
 * SUCCESSOR ORDER: the successors of a node are ordered by the position of the edges with that tail in the graph's edge
 * order (the adjacency order of the networkx graph that gfa2_reconstruct_assembly_graph builds from the E lines).
 * COUNT: with U the interior of bubble (s, t): cnt[t] = 1, cnt[v] = sum of cnt[w] over the out-edges (v, w) of every v in
 * U + {s}, in 64 bits, saturating at PO_PATHS_MANY (a sum never wraps); n_paths = cnt[s].  t may enter the next bubble: as
 * an end its count is 1.
 * PATH ORDER: path j of a bubble is the j-th in lexicographic order of successor positions -- the index j unranked through
 * the counts: at v the first successor w with j < cnt[w] once the counts of the successors before it are subtracted.  On a
 * DAG this is the list networkx.all_simple_paths gives, path for path.  A path is listed with both ends: s, .., t.  The
 * paths of a bubble are listed iff n_paths <= max_paths and the count is not saturated.
 * INTERIOR: the nodes strictly inside, ascending in rank of the node order; n_inside of them.
 * EXIT PREDECESSORS: every edge (p, t) as (p, weight), in the graph's edge order.
 * PO_PATHS_BARE: n_inside == 0.  The reference's non_branching_bubble drops a bubble iff out_degree(s) == 1, in_degree(t) == 1
 * and successors(s)[0] == t, and its walk of the chain ends at the first dropped bubble.  The three conditions hold iff the
 * interior is empty: if the only out-edge of s goes to t, no node is reached from s without passing t; and a superbubble is
 * closed -- every out-edge of s ends in U + {t}, every in-edge of t starts in U + {s} -- so with U empty s has the one
 * successor t and t the one predecessor s (an edge (u, v) is in the graph once).  DESIGN.md section 3.9r.
 * The result is of a kind of its own and stays in HBM until po_result_free.  po_paths_sizes gives the lengths; po_paths_copy
 * the arrays, any of which may be NULL: bubbles (n_bubbles); inside_off, pred_off, bubble_path_off (n_bubbles + 1 each:
 * offsets into inside_nodes, into pred_node / pred_weight, and the number of the bubble's first listed path); path_off
 * (n_listed_paths + 1, offsets into path_nodes).
 * Limits: as po_layout_bubblechains; and when the paths to list number 2^30 or more, or their nodes together reach 2^31, the
 * call fails with PO_ERR_CAPACITY and a message and writes nothing -- the first from the counts alone, before anything is
 * listed.  Device memory beyond the inputs and the result is linear: what po_layout_bubblechains takes plus at most 60 bytes
 * per node and 32 per edge (two key arrays, padded to a power of two), and 4 bytes per listed path.  The counting rounds are
 * bounded on the host by the largest n_inside + 2, the walk of a path by n_inside + 1 steps; reaching a bound is PO_ERR_HIP,
 * never a result.  Only integers are involved: every output is the same on every run.  params may be NULL (max_paths 0).
 * An empty graph: PO_OK, every size 0.  Rejections, each PO_ERR_INVALID with a message: a row result; a result of another
 * handle; reserved != 0; out NULL; an edge with an end that is not in the node order (counted in n_invalid).  There is no CPU
 * fallback: without a GPU a valid call returns PO_ERR_HIP. */
po_status po_phase_paths(po_handle* h, po_result* graph, const po_paths_params* params, po_result** out);
po_status po_paths_sizes(const po_result* out, po_paths_dims* dims);
po_status po_paths_copy(po_result* out, po_bubble_paths* bubbles, uint64_t* inside_off, uint32_t* inside_nodes, uint64_t* pred_off,
                        uint32_t* pred_node, int32_t* pred_weight, uint64_t* bubble_path_off, uint64_t* path_off, uint32_t* path_nodes);
po_status po_get_paths_stats(const po_handle* h, po_paths_stats* out);

/* ---------------------------------------------------------------------------------------------
 * The large-bubble arm of `phasm phase`: phase_large_bubble (phasm/phasing.py:633-685) on a bubble whose paths po_phase_paths
 * left listed in HBM -- every listed path scored against the relevant reads, the n_best best of them named -- for a bubble of
 * any listed size (po_phase_branch stops at 64 paths).  phasm_amd/csrc/large.hip.h, DESIGN.md section 3.9v.
 * Not part of it: the relevant reads (po_phase_relevant), the reads of a node (the caller's), spelling the winner (po_spell).
 * --------------------------------------------------------------------------------------------- */

typedef struct {
    uint32_t bubble;             /* index into the table of the paths result                                        */
    uint32_t n_reads;            /* R >= 1: the relevant reads                                                      */
    uint32_t n_b;                /* local read ids are 0..n_b-1                                                     */
    uint32_t n_best;             /* 1..8: how many of the best paths to name                                        */
    uint32_t reserved;           /* must be 0                                                                       */
} po_large_params;

typedef struct {
    const int32_t* overlap_max;  /* [n_reads]; these five are exactly those fields of po_phase_input                */
    const uint32_t* aln_off;     /* [n_reads + 1]                                                                   */
    const uint32_t* aln_b;
    const int32_t* aln_a0;
    const int32_t* aln_a1;
    const uint32_t* node_off;    /* [n_nodes + 1]: the local read ids of interior node i are node_off[i] .. node_off[i+1]-1 */
    const uint32_t* node_ids;    /* the local ids of the reads of every interior node, in the order of the bubble's
                                    inside_nodes; a merged node has several, a node whose reads no alignment names none */
    uint32_t n_nodes;            /* must be the bubble's n_inside                                                   */
} po_large_input;

typedef struct {
    uint64_t n_paths, n_inside, n_reads;
    uint64_t max_path_nodes;     /* nodes of the bubble's longest listed path, both ends included                   */
    float ms_intervals;          /* uploads, slot map, bitsets and intervals of the interior nodes                  */
    float ms_score, ms_best, ms_total;
} po_large_stats;

/* po_phase_large.  `paths` is a po_phase_paths result of this handle; it stays valid and unchanged.
 * SCORE.  For path p of the bubble (numbered as bubble_path_off numbers them, from 0 within the bubble), in float64,
 *     sum[p] = sum over the relevant reads r of f(r; the reads of the interior nodes of p),  score[p] = sum[p] / n_reads
 *   with f as in po_phase_branch.  The interval (S0, E) is kept per (interior node, read) and a path joins those of its nodes
 *   with min and max.  The sum runs in the order of po_phase_branch's table, so sum[p] has the bits of S[0][0][p] of that call
 *   with ploidy 1, one candidate and an empty read set on the same paths; the division happens on the device, once per path.
 *   A path without interior nodes (an edge from entrance to exit) scores 0.0.
 * BEST.  best_out[0 .. n-1], n = *n_best_out = min(n_best, n_paths), are the indices within the bubble that
 *   sorted(range(P), key=score.get, reverse=True)[:n_best] gives: descending by score, among equal scores the lower index
 *   first.  best_score_out[j] is score[best_out[j]].  Integer atomics on an order-keeping key, then on the index; no
 *   floating-point atomics: the same input gives the same bits on every run.
 * scores_out (may be NULL) receives all n_paths scores; nothing else of size n_paths leaves the device.
 * REJECTIONS, each PO_ERR_INVALID with a sentence in po_last_error, checked on the host before a kernel runs, the outputs
 *   untouched (*n_best_out = 0 where it is given), in this order: a NULL argument; reserved != 0; n_best outside 1..8;
 *   n_reads == 0 (the reference divides by zero there); a missing array; offsets that do not start at 0 or that decrease; a
 *   local id >= n_b; a result that is no paths result or belongs to another handle; bubble >= n_bubbles; a bubble whose paths
 *   were not listed (PO_PATHS_UNLISTED); n_nodes != the bubble's n_inside (the last two need the result's table, which comes
 *   to the host once per result).
 * Device memory beyond the inputs: 8 * n_inside * n_reads bytes for the intervals, 4 * ceil(n_b / 32) per interior node, one
 * word per node of the graph for the slot map, 8 * n_paths for the scores.  Every loop is bounded on the host.  There is no
 * CPU fallback: without a GPU a valid call returns PO_ERR_HIP. */
po_status po_phase_large(po_handle* h, po_result* paths, const po_large_params* params, const po_large_input* input,
                         uint64_t* best_out, double* best_score_out, double* scores_out, uint32_t* n_best_out);
po_status po_get_large_stats(const po_handle* h, po_large_stats* out);

/* The listed paths first .. first + count - 1 of a po_phase_paths result, numbered as bubble_path_off numbers them:
 * path_off_out[0 .. count] are offsets into path_nodes_out RELATIVE to the first path (path_off_out[0] = 0), path_nodes_out the
 * nodes, both ends of each path included.  *n_nodes_out is always the number of nodes of the range; cap is the room of
 * path_nodes_out in nodes.  Either array may be NULL (cap is ignored without path_nodes_out).  Rejections: PO_ERR_INVALID
 * for a NULL result or n_nodes_out, a result that is no paths result, a range that ends past the listed paths;
 * PO_ERR_CAPACITY, with *n_nodes_out set and nothing written, when cap is too small. */
po_status po_paths_copy_paths(po_result* paths, uint64_t first, uint64_t count, uint64_t* path_off_out, uint32_t* path_nodes_out,
                              uint64_t cap, uint64_t* n_nodes_out);

/* ---------------------------------------------------------------------------------------------
 * The walk of `phasm phase` along a bubble chain with the candidate sets RESIDENT on the device: what
 * BubbleChainPhaser carries from bubble to bubble (candidate_sets with their read sets and log_rl, phasm/phasing.py:125-142),
 * the take-over of the survivors (phasing.py:311-319), new_block's reset (phasing.py:343-364) and prune(.., 1.0) of new_block
 * and of the end of phase() (phasing.py:335-339, 347).  phasm_amd/csrc/walk.hip.h, DESIGN.md section 3.9s.
 * Not part of it: the loop itself and its arms (phasm_amd/phasing.py, phase_chain), prev_graph_reads / prev_aligning_reads
 * (host lists of the caller on this route; the walk's own on the resident route further down), the choice among ties.
 * --------------------------------------------------------------------------------------------- */

typedef struct {
    uint32_t ploidy;             /* k of po_walk_create                                                             */
    uint32_t n_cands;            /* the candidate sets of the state; 1 after po_walk_create and po_walk_reset       */
    uint32_t depth;              /* bubbles advanced since the reset                                                */
    uint32_t start_of_block;     /* depth == 0                                                                      */
    uint64_t n_block_reads;      /* reads that a step since the reset named in b_reads and then advanced            */
} po_walk_info;

typedef struct {
    uint64_t n_cands_in, n_cands_out;   /* candidates before the step and after it (equal where it did not advance) */
    uint64_t depth, n_block_reads;      /* after the step                                                           */
    uint64_t n_new_reads;        /* reads of b_reads that were new to the block (they joined it iff the step advanced) */
    uint32_t words_per_slot;     /* W of the state's rows after the step                                            */
    uint32_t advanced;           /* the step took its final list over                                               */
    float ms_bits;               /* path bitsets and the intervals of slots and paths (ms_intervals of the phase stats) */
    float ms_advance;            /* k_wk_advance                                                                    */
    float ms_total;              /* ms_total of the phase stats + ms_advance + ms_resident                          */
    float ms_resident;           /* po_walk_step_resident: the k_rs_ kernels (new reads and their scan, the translation
                                    of aln_b and of the path ids, the commit of the map and of the two sets); 0 after
                                    po_walk_step                                                                    */
} po_walk_stats;

/* A WALK is a result of a kind of its own: it belongs to one handle, po_result_count is 0, po_result_free frees it; every
 * call that wants rows, candidates, edges or another special result refuses it.  Creating, resetting and asking a walk that
 * has not advanced touch no device.
 * po_walk_create: ploidy 1..8.  The state is that of BubbleChainPhaser.__init__ / new_block: ONE candidate with k empty
 *   read sets and log_rl = -inf, depth 0, no block reads, start of block.
 * po_walk_reset: back to that state (the reset half of new_block; its prune(.., 1.0) is po_walk_best, called before).
 * po_walk_step: po_phase_branch on the bubble whose read-set list c * k + i is: the interior reads of every path that slot i
 *   of candidate c took at the advanced bubbles of the block, as far as they are in b_reads.  params and input are those of
 *   po_phase_branch except: input.set_off and input.set_ids must be NULL; params.n_cands must equal the walk's count,
 *   params.start_of_block its flag, params.ploidy its ploidy (a caller whose idea of the state has drifted is told).
 *   b_reads[params.n_b]: the global oriented read ids behind the local ids 0..n_b-1, strictly ascending, as po_relevant_copy
 *   gives them.  The entries, their order, every level of prune and po_get_phase_stats are those of po_phase_branch; since
 *   (S0, E) are a least and a greatest value and the table's sums run over the relevant reads in index order, neither of
 *   which the numbering of the b reads touches, (cand, ext, rl) are byte-equal to po_phase_branch's on the same handle.  A
 *   block read that b_reads leaves out can match nothing.
 *   advance != 0 and at least one entry in the final list: the state becomes that list -- candidate j takes over slot i of
 *   candidate cand[j] and adds to it the interior of path digit_i(ext[j]) (digits base P, slot 0 most significant), its
 *   log_rl is rl[j]; depth grows by 1; the reads of b_reads that are new to the block join the block reads.  advance == 0,
 *   or no entry: the state is untouched (advance == 0 is the peek a callable prune factor needs).
 *   cap bounds only what is copied home: *n_out is always the full count, and the state takes the whole list.
 *   Rejections as po_phase_branch's (PO_ERR_INVALID with a sentence, checked on the host before the device is touched,
 *   outputs and state untouched), and: a walk of another handle or a result of another kind; non-NULL set_off / set_ids; the
 *   three mismatches; b_reads NULL with n_b > 0, or not strictly ascending.  A call that fails later (PO_ERR_HIP,
 *   PO_ERR_NOMEM) leaves the state as it was.
 * po_walk_best: prune(candidate_sets, 1.0) with its early returns -- fewer than two candidates, or greatest log_rl = -inf:
 *   every candidate; else the candidates with log_rl - max >= log10(1.0), ascending (no further round: 1.0 < 1.0 is false).
 *   Up to cap of them go to cands_out, *n_out is the full count, *max_rl_out (may be NULL) the greatest log_rl.
 * po_walk_history: for each of the n named candidates its extension id at every advanced bubble of the block,
 *   ext_out[q * depth + d], oldest first (room for n * depth entries).
 * po_walk_read_sets: the k read sets of each named candidate as global read ids, ascending, in CSR form: off_out[n * k + 1],
 *   up to cap ids to ids_out, *n_ids_out the full count.  For the yielded block and for tests: the bit rows of the named
 *   candidates come home and are expanded on the host.
 * A candidate >= n_cands, a NULL count: PO_ERR_INVALID.  There is no CPU fallback: without a GPU a valid step returns
 * PO_ERR_HIP.  Device memory of a walk: 2 x 4 W bytes per slot, 2 x 8 per candidate, 8 per survivor of every advanced bubble. */
po_status po_walk_create(po_handle* h, uint32_t ploidy, po_result** walk_out);
po_status po_walk_reset(po_result* walk);
po_status po_walk_info_get(const po_result* walk, po_walk_info* info);
po_status po_walk_step(po_handle* h, po_result* walk, const po_phase_params* params, const po_phase_input* input, const uint32_t* b_reads,
                       uint32_t advance, uint32_t* cand_out, uint32_t* ext_out, double* rl_out, uint64_t cap, uint64_t* n_out);
po_status po_walk_best(po_result* walk, uint32_t* cands_out, uint64_t cap, uint64_t* n_out, double* max_rl_out);
po_status po_walk_history(po_result* walk, const uint32_t* cands, uint64_t n, uint32_t* ext_out);
po_status po_walk_read_sets(po_result* walk, const uint32_t* cands, uint64_t n, uint64_t* off_out, uint32_t* ids_out, uint64_t cap,
                            uint64_t* n_ids_out);
po_status po_get_walk_stats(const po_handle* h, po_walk_stats* out);

/* THE RESIDENT ROUTE through one step of the walk (phasm_amd/csrc/resident.hip.h): the gather and the
 * step of one bubble without the host between them.  Per bubble only the interior reads, the exit predecessors and the path
 * reads (global ids) go up; only the sizes of the gather and the (cand, ext, rl) list come home.  po_walk_step stays as it is.
 * The walk owns two bitsets over the handle's read ids, prev_graph and prev_aligning (ceil(n_ids / 32) words each), empty
 * after po_walk_create and po_walk_reset, and the map of the block-stable ids on the device: stable_of[global id] (4 bytes per
 * read of the handle) and global_of[stable id].  Creating and resetting still touch no device: what a reset has to clear is
 * cleared at the next device call, the map over the old block's reads alone.
 * po_walk_relevant: the gather of po_phase_relevant with prev_graph and prev_aligning taken from the walk
 *   (input.prev_graph / prev_aligning must be NULL with count 0).  without_prev_graph != 0 takes prev_graph as empty (what the
 *   walk does at a large bubble); prev_aligning still counts toward n_spanning.  The arrays, the bitsets of cur_graph and
 *   cur_aligning and the ranks of G stay in device buffers of the WALK (no other call on the handle overwrites them).  *out is a
 *   result of the kind po_phase_relevant returns: po_relevant_sizes works at once, po_relevant_copy fetches the arrays from the
 *   device and gives byte for byte what po_phase_relevant gives for the same sets passed as lists.  A walk holds ONE live
 *   gather: the next po_walk_relevant on it, a po_walk_reset (but see below) or the freeing of the walk makes the earlier
 *   result stale; po_relevant_copy and the step refuse a stale result (PO_ERR_INVALID with a sentence).  It is freed with
 *   po_result_free like any result, before or after its walk.  po_get_relevant_stats: the sizes; ms_alignments is 0 and
 *   ms_total ends where the lists are made, because the last launches are not waited for.
 * po_walk_step_resident: po_walk_step on the gather `rel`.  Of input only path_off, path_ids -- GLOBAL read ids -- and levels
 *   are given, every other pointer must be NULL.  params.n_reads and params.n_b must equal the gather's n_relevant and n_b;
 *   n_cands, ploidy and start_of_block the walk's.  rel must be the walk's live gather, made at the walk's present depth; one
 *   exception: a gather with fell_back (or made with mode 1) is accepted after ONE po_walk_reset (new_block() followed by the
 *   step on the same relevant reads).  A path id that is not in the gather's b_reads is dropped.  The block-stable ids follow
 *   the rule of po_walk_step: a read known to the block keeps its id, the reads of b_reads new to the block get n_block + their
 *   rank among the new ones in the order of b_reads; so (cand, ext, rl), the state and the stats are those of po_walk_step on
 *   the same arrays.  Commit rule as po_walk_step's: advance == 0 or an empty final list changes nothing -- not the candidates,
 *   not the map, not the two sets -- so a peek followed by the advancing call on the same rel numbers the new reads
 *   identically.  A step that advances also joins cur_graph to prev_graph and cur_aligning to prev_aligning.
 *   ONE ROUTE PER BLOCK: after a block's first advancing step by one route, the other route's step -- and after po_walk_step
 *   also po_walk_relevant -- is refused until po_walk_reset.  po_walk_info_get, po_walk_best, po_walk_history and
 *   po_walk_read_sets work on either route (po_walk_read_sets brings global_of home when asked).
 * po_walk_prev_copy: prev_graph (which 0) or prev_aligning (which 1) as an ascending list, up to cap ids; *n_out is the full
 *   count.
 * Rejections, each PO_ERR_INVALID with a sentence, decided on the host before the device is touched, outputs and state
 * untouched: NULL out / n_out, walk, index, rel, params or input; reserved != 0; mode > 1; non-NULL previous lists; an id >=
 * po_num_sequences; a walk, index or rel of another handle or of another kind; a stale rel; any po_phase_input pointer other
 * than the three being non-NULL; the five mismatches (n_reads, n_b, ploidy, n_cands, start_of_block) and a gather of another
 * depth; the other route inside a block; which > 1.  There is no CPU fallback: without a GPU a valid call returns PO_ERR_HIP. */
typedef struct {
    uint32_t mode;               /* as po_relevant_params                                                           */
    uint32_t min_spanning_reads;
    uint32_t without_prev_graph; /* non-zero: prev_graph counts as empty                                            */
    uint32_t reserved;           /* must be 0                                                                       */
} po_walk_relevant_params;
po_status po_walk_relevant(po_handle* h, po_result* walk, po_result* index, const po_walk_relevant_params* params,
                           const po_relevant_input* input, po_result** out);
po_status po_walk_step_resident(po_handle* h, po_result* walk, po_result* rel, const po_phase_params* params, const po_phase_input* input,
                                uint32_t advance, uint32_t* cand_out, uint32_t* ext_out, double* rl_out, uint64_t cap, uint64_t* n_out);
po_status po_walk_prev_copy(po_result* walk, uint32_t which, uint32_t* ids_out, uint64_t cap, uint64_t* n_out);

/* A graph that did not come from po_layout_edges: `edges` over the handle's oriented reads (2i / 2i+1 of segment i of
 * po_add_segment or po_add_sequence) and the order of its nodes.  Checked on the host before anything touches the
 * device, each violation PO_ERR_INVALID with a message: u, v < po_num_sequences; node_order entries in range and
 * distinct; every edge end present in node_order; the (u, v) pairs distinct.  The result works with po_result_count,
 * po_result_rows, po_result_node_order, po_result_free and po_layout_components; po_layout_reduce, _tips, _diamonds,
 * _merge and _coverage refuse it with PO_ERR_INVALID.  Without a GPU a valid call returns PO_ERR_HIP. */
po_status po_graph_from_edges(po_handle* h, const po_edge* edges, uint64_t n_edges, const uint32_t* node_order,
                              uint64_t n_order, po_result** out);

/* The nodes of an edge result's graph in the reference's order (`for n in g`: the order in which add_edge first saw
 * each node, phasm/assembly_graph.py:136-179, without the nodes of contained reads), computed by po_layout_edges from
 * the rows: a row reaches build_assembly_graph iff it passes the filters and no earlier row has marked one of its
 * oriented reads contained (ContainedReads is stateful, phasm/filter.py:90-101); it inserts a, b, b^1, a^1
 * (OVERLAP_AB) or b, a, a^1, b^1 (OVERLAP_BA).  *n_out = number of nodes; up to `cap` of them go to nodes_out. */
po_status po_result_node_order(po_result* r, uint32_t* nodes_out, uint64_t cap, uint64_t* n_out);

/* What the node order cost the last po_layout_edges call: two passes over the rows that run on every call, behind the
 * times of po_layout_stats (whose ms_total does not include them). */
typedef struct {
    uint64_t n_rows;
    float ms_first_contained;    /* first containing row per oriented node (with the memsets)                     */
    float ms_rank;               /* first reaching (row, slot) per node                                           */
    float ms_total;
} po_node_order_stats;
po_status po_get_node_order_stats(const po_handle* h, po_node_order_stats* out);

/* Diagnostics for the test suite (no reference counterpart: addSequence copies its argument and
 * never touches it again, src/overlapper.cpp:22-26 -- these two calls let a test PROVE that of this library).
 * po_debug_host_ranges: every range of host memory the library has made visible to the GPU in this process, ever
 * (hipHostMalloc'ed landing zones and result arrays, the hipHostRegister'ed packed read stores): `out` receives up to
 * cap_entries triplets {base, bytes, kind} (kind & 0xFF: 1 = page-locked allocation, 2 = registered store; bit 8: still
 * live); returns the number of entries on the list.  Device->host copies and host-mapped stores of the library can
 * only land inside these ranges.
 * po_debug_pointer_info: what the HIP runtime (hipPointerGetAttributes -> *hip_type, -1 = unknown to it) and the ROCr
 * runtime underneath (hsa_amd_pointer_info -> *hsa_type: 0 unknown, 1 runtime allocation, 2 locked / registered host
 * memory; -1 = not queried) know about address p, and the range they know it as.  Returns 1 if either knows it -- i.e.
 * the GPU can address that page -- else 0.
 * po_debug_fault_backtrace: install a SIGSEGV / SIGBUS handler that writes the faulting address and the native stack of
 * the faulting thread to `fd`, then runs whatever handler was installed before it (a store into a read-only input mapping
 * by a thread that has no Python frames -- a runtime thread -- is named this way).  Returns 0 on success. */
uint64_t po_debug_host_ranges(uint64_t* out, uint64_t cap_entries);
/* po_debug_store_words: the packed host store `store` (0: reads of even index, 1: odd) as it stands -- *words points into the
 * handle (valid until the next call that adds reads), returns the number of 8-byte words.  Tests compare the stores the
 * parallel FASTA ingest writes with the ones po_add_sequence builds. */
uint64_t po_debug_store_words(const po_handle* h, int store, const uint64_t** words);
/* The host half of po_overlaps_to_host's compact row transfer on its own, for tests without a GPU: the rows of `n`
 * verified-candidate records (po_cand; one per strand-mirror pair when paired != 0), written by the library's helper
 * threads in the order po_overlaps emits them -- A row, [its mirror], B row, [its mirror] per record (row fields:
 * src/overlapper.cpp:77-82,104-110; mirror rules: SURVEY.md section 8c).  0 = ok; 1 = the rows differ in number from
 * n_rows_expected (nothing reliable was written); 2 = a record names a read >= n_reads; -1 = no helper thread. */
int po_debug_expand_records(const po_cand* records, uint64_t n, const uint32_t* lengths, uint32_t n_reads, uint32_t paired,
                            po_row* rows_out, uint64_t n_rows_expected);
/* ... and of `n` records of EIGHT bytes, a | b << sh_b | p << sh_p | type << 62 (what po_overlaps_to_host sends when the
 * read set fits: 2 ceil(log2 reads) + ceil(log2 (longest read + 1)) <= 62); -2 = shifts out of range. */
int po_debug_expand_packed(const uint64_t* records, uint64_t n, uint32_t sh_b, uint32_t sh_p, const uint32_t* lengths, uint32_t n_reads,
                           uint32_t paired, po_row* rows_out, uint64_t n_rows_expected);
int po_debug_fault_backtrace(int fd);
int po_debug_pointer_info(const void* p, int32_t* hip_type, int32_t* hsa_type, uint64_t* base, uint64_t* bytes);

po_status po_get_stats(const po_handle* h, po_stats* out);
const char* po_last_error(const po_handle* h);
int po_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PHASM_OVERLAP_H */
