/*
 * hyperball.h - C ABI of the MI355X-native HyperBall harmonic-centrality library.
 *
 * Drop-in boundary.  The reference call site is
 *
 *     crates/core/src/entrypoint/centrality.rs:46-53
 *         let graph = WebgraphBuilder::new(path, 0).open();
 *         let hc    = HarmonicCentrality::calculate(&graph);          // harmonic.rs:292
 *         store_harmonic(hc.iter().map(|(n, c)| (*n, c)), out);       // centrality/mod.rs:72
 *
 * A Rust shim keeps `pub struct HarmonicCentrality(BTreeMap<NodeID,f64>)`
 * (harmonic.rs:289-311) and replaces the body of `calculate` by:
 *     hb_create -> hb_load_edges(graph.host_nodes(), graph.host_edges()) -> hb_run
 *     -> hb_result_count / hb_result_copy -> BTreeMap -> hb_destroy.
 * Everything upstream (Webgraph loader) and downstream (speedy_kv centrality store
 * writer) is untouched.
 *
 * All functions are extern "C", never unwind, keep no global state.  One host thread
 * per context; calls on one context are not re-entrant.  Return value: 0 = HB_OK,
 * negative = error (message via hb_last_error).  The library needs a gfx950 GPU; there
 * is NO CPU fallback - every entry point that computes fails with HB_ERR_NO_DEVICE
 * when no device is present.
 */
#ifndef HYPERBALL_H
#define HYPERBALL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HB_ABI_VERSION 6 /* 6 [r6]: hb_options.tune[1] above its low byte and tune[7] are refused by the product library (experiments build
                            only); layouts unchanged since 5 */

/* ---- error codes -------------------------------------------------------------- */
#define HB_OK 0
#define HB_ERR_INVALID   (-1) /* bad argument / call order                         */
#define HB_ERR_NO_DEVICE (-2) /* no HIP device, or not gfx950                      */
#define HB_ERR_HIP       (-3) /* a HIP runtime call failed                         */
#define HB_ERR_NOMEM     (-4) /* host or device allocation failed                  */
#define HB_ERR_RCCL      (-5) /* an RCCL call failed                               */
#define HB_ERR_LIMIT     (-6) /* n >= 2^30 nodes, or max_passes exceeded            */
#define HB_ERR_IO        (-7) /* a file could not be created / written (hb_store.h) */

/* ---- plain data ---------------------------------------------------------------- */

/* Rust `u128` <-> two little-endian u64 halves.  NodeID(u128): webgraph/node.rs:37.
 * Ordering everywhere is the numeric u128 order (hi first, then lo). */
typedef struct hb_u128 {
    uint64_t lo;
    uint64_t hi;
} hb_u128;

/* SmallEdge { from: NodeID, to: NodeID, rel_flags: RelFlags(u64) }, webgraph/edge.rs:31-35;
 * 40 bytes, #[repr(C)] on the Rust side. */
typedef struct hb_edge {
    hb_u128 from;
    hb_u128 to;
    uint64_t rel_flags;
} hb_edge;

/* Edges with rel_flags & HB_SKIPPED_REL_MASK != 0 are dropped (after first-occurrence
 * de-duplication): SKIPPED_REL, harmonic.rs:36-49, bit values
 * webpage/html/links.rs:114-141. */
#define HB_SKIPPED_REL_MASK 0x6FED00ull

/* ---- options ------------------------------------------------------------------- */
#define HB_FLAG_NO_FRONTIER   0x01u /* never skip unchanged sources (debug; same results)          */
#define HB_FLAG_NO_REORDER    0x02u /* keep ascending-NodeID order as the device order            */
#define HB_FLAG_UNFUSED       0x04u /* run merge and estimator/Kahan as two kernels even on 1 GPU  */
#define HB_FLAG_PASS_STATS    0x08u /* also count active edges / touched rows per pass (A_t, V_t)  */
#define HB_FLAG_NO_XCD_MAP    0x20u /* plain blockIdx -> tile mapping, no XCD-affine chunk groups  */
#define HB_FLAG_NO_RCCL       0x40u /* world_size > 1 bookkeeping without a communicator: the caller
                                       performs the exchange (hb_debug_exchange; tests)       */
#define HB_FLAG_NO_SPARSE     0x100u /* never use the data-driven sweep passes (debug; same results)       */
#define HB_FLAG_DEST_PARTITION 0x200u /* world_size > 1: destination partition instead of edge partition -
                                        rank r owns the nodes whose rank in ascending NodeID order is
                                        r mod world_size and must be given ALL in-edges of those nodes
                                        (records for other nodes are ignored); one ncclAllGather of the
                                        owned counter slices per pass instead of an all-reduce          */
#define HB_FLAG_HOST_INGEST   0x400u /* hb_load_edges: reduce the records on the host (hb_host.cpp) instead of
                                        on the GPU (hb_ingest.hip); same result                      */
#define HB_FLAG_HOST_PLAN     0x800u /* build the device work layout on the host (hb_host.cpp) instead of on the GPU
                                        (hb_plan.hip); same layout, also for the destination partition                     */
#define HB_FLAG_CHANGED_ONLY  0x1000u /* with HB_FLAG_DEST_PARTITION: after the changed bits (all-gather) only the counters that
                                         changed in the pass travel (one ncclBroadcast of its packed run per rank) instead of
                                         the all-gather of whole slices: ~18 % fewer bytes in the dense passes of the R-MAT
                                         configs, ~100 % fewer in the tail; same results.
                                         With the edge partition: the ranks' "my local merge changed this row" bitmaps are
                                         all-gathered and OR-ed, and the ncclAllReduce(max, u8) runs over the rows of that union
                                         only (packed in the same order on every rank) instead of all n counters */
#define HB_FLAG_REFERENCE_TAIL 0x2000u /* reproduce the reference's changed-node machinery AS WRITTEN instead of its host-level
                                          meaning: the bloom filter of changed nodes with its false
                                          positives (harmonic.rs:221-225,133; bloom/src/lib.rs:85-123), the exact-counting
                                          switch (:277-279) and, once 0 < |changed| <= round(sqrt(n)), update_changed_counters
                                          (:75-114), which follows the PAGE-level records a ForwardlinksQuery on the host id
                                          returns (query/forwardlink.rs:95-101,153-173) - give them with hb_load_tail_edges.
                                          On a graph whose pages are hosts this equals the default; on a real crawl it is
                                          what `stract centrality harmonic` prints.  Single rank only; passes run unfused. */
#define HB_FLAG_NO_INIT_PASS  0x4000u /* pass 0 like every other dense pass (64-byte gathers) instead of streaming the sources'
                                         single initial register with the edge list (2 bytes per edge, written at load time);
                                         same results, measurement switch */
#define HB_FLAG_ALL_RELS      0x8000u /* every edge record is an edge: no SKIPPED_REL filter at ingest (then m_eff == m_unique).  The page
                                          graph of ApproxHarmonic follows every ForwardlinksQuery edge (query/forwardlink.rs:44-53); use
                                          with hb_sampled_harmonic.  Not with HB_FLAG_REFERENCE_TAIL                                     */
#define HB_FLAG_LIVE_FIRST    0x10000u /* device order "live hosts first": the hosts with >= 1 in-edge by descending out-degree, then the
                                          hosts WITHOUT an in-edge ("dead": their counter never changes after hb_begin) in the same order
                                          among themselves.  From pass 1 on the dense passes do not gather dead sources (pass 0 has merged
                                          their one register into every reader) and the node-row launches of the dense and bitmap passes
                                          end at the last live row; same results, same per-pass statistics.
                                          The order is used where the argument holds for the whole graph: one rank, no communicator, no
                                          destination partition, fused passes, neither HB_FLAG_PASS_STATS nor HB_FLAG_NO_REORDER - every
                                          other context ignores both flags and plans as before.  Default: on when n >= 2^20.  This flag
                                          forces it on for smaller graphs, HB_FLAG_NO_LIVE_FIRST off for larger ones (tests, A/B runs)  */
#define HB_FLAG_NO_LIVE_FIRST 0x20000u /* never use the live-first order (wins over HB_FLAG_LIVE_FIRST)                               */
#define HB_FLAG_NO_SATURATION 0x40000u /* dense passes gather for every row.  Default (off): a node row whose counter is, register by
                                          register, at least U - the maximum over the initial counters of the hosts with an out-link -
                                          can never change again; from then on the dense passes t >= 1 neither gather for it nor compute
                                          the hub chunks below it.  Same results and per-pass statistics (`touched`
                                          of a bitmap pass may differ on split rows, as between two layouts).  Used where the argument
                                          holds for the whole graph: one rank, no communicator, no destination partition, fused passes,
                                          no HB_FLAG_PASS_STATS - every other context runs as with this flag (tests, A/B runs)        */
#define HB_FLAG_NO_EARLY_EXIT  0x80000u /* a dense pass gathers every source of every row it gathers for.  Default (off), in the contexts
                                          that skip saturated rows: once the rows saturated so far in the run hold at least 1/64 of the
                                          edges as sources, the dense passes leave a row's (or hub chunk's) gather loop after the round in
                                          which its accumulator has reached U - no later source can raise it.  Same
                                          results and statistics.  HB_FLAG_NO_SATURATION implies this flag (tests, A/B runs)             */
#define HB_FLAG_FORCE_EARLY_EXIT 0x100000u /* those dense passes test for the early exit from pass 1 on, whatever is saturated (tests: small
                                          graphs reach the code in passes where nothing is saturated yet).  Same results; loses to
                                          HB_FLAG_NO_EARLY_EXIT and HB_FLAG_NO_SATURATION                                                  */
#define HB_FLAG_PACKED_WIRE   0x200000u /* every exchange that moves WHOLE counters moves them as 48-byte packed rows: a plain
                                          little-endian bit stream of 64 six-bit codes, code = r for r <= 58 and 63 for r == 65 (a
                                          register of this library is 0, 1..58 or 65, so the packing is exact).  The destination
                                          partition's all-gather ships S x 48 bytes per rank; the edge partition's all-reduce(max) - plain
                                          and HB_FLAG_CHANGED_ONLY - becomes: pack, all-to-all of the ranks' slices, maximum of the
                                          received pieces, all-gather of the packed slices, unpack (0.75 x the bytes, same results; the
                                          per-range pipeline of the plain form is off).  The destination partition's changed-only
                                          exchange is packed already and does not change.  A context without a communicator and without
                                          caller collectives (one rank, no HB_FLAG_RCCL_SELF) ignores the flag.  Not with
                                          HB_FLAG_REFERENCE_TAIL.  With hb_set_collectives on the edge partition: hb_set_all_to_all too
                                           */
#define HB_FLAG_RCCL_SELF     0x80u /* world_size == 1 but still create a 1-rank communicator and run
                                       the collectives (exercises the RCCL call path on one GPU)   */

typedef struct hb_options {
    uint32_t struct_size;   /* = sizeof(hb_options); 0 is accepted as "this version"       */
    int32_t  device;        /* HIP device ordinal; < 0 = current device                     */
    uint32_t flags;         /* HB_FLAG_*                                                   */
    uint32_t chunk;         /* max sources per work row (hub rows are split); 0 = default  */
    uint32_t max_passes;    /* safety bound on passes; 0 = 4096                            */
    int32_t  rank;          /* edge-partition mode: this process' rank ...                 */
    int32_t  world_size;    /* ... of world_size (<= 1: single GPU, no collective)         */
    uint8_t  rccl_id[128];  /* ncclUniqueId from hb_rccl_unique_id() of rank 0             */
    uint32_t tune[8];       /* tuning knobs, 0 = default (every setting gives the same results; these only move time):
                             *  [0] workgroups per CU of the pass launches: low byte = node rows (dense 64, bitmap 32),
                             *      second byte = hub chunks (dense 2, bitmap 5)
                             *  [1] low byte: gather unroll 1|2|4 (hub chunks 4, node rows 2).  The bits above it are switches of the
                             *      experiments build only (stract_amd/csrc/hb_experiments.h); hb_create refuses them
                             *  [2] bitmap passes when A_t < tune[2] % of the edges (50; > 100 = always)
                             *  [3] log2 of the hotness slice width in counters (16 = 4 MiB; 1 = no slices)
                             *  [4] min sources of a chunk at a slice cut (8)
                             *  [5] largest row that is not split into chunks (chunk)
                             *  [6] sweep passes (touched rows only) when A_t * tune[6] < edges (10; 1 = whenever a bitmap pass would run)
                             *  [7] reserved, must be 0 (experiments build: see hb_experiments.h)                 */
} hb_options;

typedef struct hb_ctx hb_ctx;

/* ---- statistics ------------------------------------------------------------------ */
typedef struct hb_stats {
    uint64_t n;             /* |V| (harmonic.rs:58-72)                                     */
    uint64_t m_input;       /* edge records received                                       */
    uint64_t m_unique;      /* unique (from,to) pairs (store.rs:313)                        */
    uint64_t m_eff;         /* ... surviving the rel-flag filter (harmonic.rs:131)          */
    uint64_t passes;        /* T, including the final no-change pass (harmonic.rs:237-240)  */
    uint64_t results;       /* nodes with centrality > 0                                    */
    double   ms_ingest;     /* host: dedup / remap / CSR build                              */
    double   ms_plan;       /* host: device ordering, hub-row splitting                     */
    double   ms_h2d;        /* graph upload + state initialisation                          */
    double   ms_loop;       /* wall time of the iteration loop (the timed quantity)         */
    double   ms_loop_gpu;   /* sum of per-pass GPU time (HIP events on the ctx stream)      */
    double   ms_collective; /* part of ms_loop_gpu spent in RCCL collectives                */
    double   ms_d2h;        /* result download + id mapping                                 */
    uint64_t work_rows;     /* real + virtual (hub-chunk) rows                              */
    uint64_t virtual_rows;
    uint64_t device_bytes;  /* device memory held by the context                            */
    uint64_t virtual_edges; /* entries of the virtual rows' source lists, all levels        */
    uint64_t levels;        /* virtual levels = hub-kernel launches per pass                */
    uint64_t level1_edges;  /* REAL edges gathered by the level-1 hub-chunk launch (the dominant kernel) */
    uint64_t level1_rows;   /* hub-chunk rows of level 1 (padding rows excluded)            */
    uint64_t direct_edges;  /* REAL edges gathered directly by the node-row launch          */
    uint64_t rows_with_in_edges; /* nodes with >= 1 in-edge: V_t of a dense pass t >= 1      */
    uint64_t wire_bytes;    /* counter + changed-bit bytes this rank received in the collectives of the last run
                               (what HB_FLAG_CHANGED_ONLY reduces), both decompositions               */
    uint64_t ingest_peak_bytes; /* high-water mark of the device memory the GPU ingest NEEDED: live record chunks,
                                   endpoint table and work arrays (0 = host ingest / hb_load_dense)   */
    uint64_t pool_peak_bytes;   /* [ABI 4] high-water mark of what the library's caching device allocator (hb_pool.h) HELD
                                   from the runtime during the load: the live bytes plus freed extents it kept for reuse
                                   (kept only while the device has room: above half of the device memory - or
                                   HB_POOL_LIMIT_BYTES - free blocks go back to the runtime before a new one is taken) */
    uint64_t result_stages;     /* [ABI 5] snapshots of the per-node sums that went to the host WHILE the passes of the last run
                                   were still running (second stream; single rank, n >= 2^20): hb_finish then ships only ... */
    uint64_t result_list;       /* [ABI 5] ... this many (node, value) entries that still moved afterwards (0 stages: the whole
                                   n x 8-byte image is downloaded by hb_finish, as before)                                      */
    uint64_t pipelined_passes;  /* [ABI 5] passes of the last hb_run that were queued BEFORE the host had read the previous pass'
                                   counters (convergence tail, one rank: a pass that changed <= 4096 nodes in sweep mode is
                                   followed by passes guarded on the device; the pass behind the loop's last one does nothing) */
    uint64_t tail_kernel_passes; /* [ABI 5] always 0 in the product library (experiments build: passes one single-workgroup launch ran
                                   from work lists; measured no faster than the launches it replaces, so not shipped)          */
} hb_stats;

typedef struct hb_pass_stats {
    uint64_t pass;          /* t                                                            */
    uint64_t changed;       /* nodes whose counter changed in pass t                        */
    uint64_t active_edges;  /* A_t = edges whose source changed in pass t-1 (out-degree sum of those
                               nodes; with HB_FLAG_PASS_STATS counted edge by edge in frontier passes) */
    uint64_t touched;       /* frontier / sparse passes: node rows with >= 1 gathered source (<= V_t: a split
                               row counts only when one of its partials changed); dense passes: 0   */
    uint32_t mode;          /* 0 = dense (no frontier test), 1 = frontier bitmap, 2 = sweep (touch bitmap of the rows
                               that read a changed node; only those rows run), 3 = reference tail
                               (HB_FLAG_REFERENCE_TAIL: update_changed_counters over the page-level records)  
                               (4 = experiments build only: the pass ran inside the single-workgroup tail kernel)                 */
    float    ms_gpu;        /* GPU time of the pass (all its launches + collective)         */
    float    ms_main;       /* GPU time of the dominant launch (real rows)                  */
    float    ms_collective;
    float    ms_level1;     /* GPU time of the level-1 hub-chunk launch (dense / frontier passes); sweep passes: of the
                               seed collection + expansion launches (then ms_main = node rows, the rest = virtual levels) */
    uint32_t reserved;
} hb_pass_stats;

/* ---- lifecycle --------------------------------------------------------------------- */
int  hb_abi_version(void);
/* opt may be NULL (defaults, current device). */
int  hb_create(const hb_options *opt, hb_ctx **out);
void hb_destroy(hb_ctx *ctx);
/* Message of the last failing call on ctx (or of hb_create when ctx == NULL). */
const char *hb_last_error(const hb_ctx *ctx);
/* [ABI 5] The library allocates device memory through a caching allocator (freed extents are kept for the next load: hipMalloc /
 * hipFree cost ~60 ms per GB cycled on these boxes); other allocators in the process (RCCL, torch, rocPRIM users) cannot reclaim
 * what it holds on their own out-of-memory.  This returns every cached block of the CURRENT device that no context uses to the
 * runtime (hb_destroy does the same); *released = bytes given back (may be NULL). */
int hb_release_cached_memory(uint64_t *released);

/* ---- graph input --------------------------------------------------------------------- */
/* Replaces the per-pass `graph.host_nodes()` / `graph.host_edges()` streaming
 * (webgraph/mod.rs:157,192 -> store.rs:297-357) by one hand-over.
 *   node_ids: graph.host_nodes() in any order, duplicates allowed; NULL/n = 0 -> the node
 *             set is derived from the endpoints of ALL edge records, flagged ones included
 *             (store.rs:338-357).
 *   edges:    graph.host_edges() order matters: the FIRST record of each (from,to) pair
 *             wins (itertools::unique_by, store.rs:313), THEN records with
 *             rel_flags & HB_SKIPPED_REL_MASK are dropped (harmonic.rs:131).  Records whose
 *             endpoint is not in the node set are ignored (harmonic.rs:135).
 * Buffers are copied; the caller may free them on return.  In edge-partition mode every
 * rank passes the full node set and its own subset of the records; all records of one
 * (from,to) pair must go to the same rank, in stream order. */
int hb_load_edges(hb_ctx *ctx, const hb_u128 *node_ids, uint64_t n, const hb_edge *edges,
                  uint64_t m);
/* Streamed variant for callers that cannot (or need not) hold all records: append any number of batches in stream
 * order, then finalize (node_ids as above).  Every batch is uploaded at once and reduced as it arrives: each endpoint
 * is looked up in / added to a device hash table that maps NodeIDs to 32-bit provisional ids, and the record stays
 * resident as (from id, to id) + 1 flag byte = 9 bytes, in chunks (no reallocation as the stream grows); nothing is
 * buffered on the host, so the caller's peak memory is one batch.  There is no record-count limit (round 3: 2^32 - 256;
 * stream positions are no longer stored - the stable sort keeps the stream order of equal pairs).  Device memory: 9 B
 * per record + 20 B per table slot (load factor <= 1/2) while the stream is held, 16-17 B per record + ~40 B per node at
 * hb_finalize (hb_stats.ingest_peak_bytes reports the high-water mark).  With HB_FLAG_HOST_INGEST, or if the device
 * runs out of memory mid-stream, the records are buffered on the host instead (same result).  Batches in pinned host
 * memory (hipHostMalloc / hipHostRegister) cross the link asynchronously at its full rate. */
int hb_append_edges(hb_ctx *ctx, const hb_edge *edges, uint64_t m);
int hb_finalize(hb_ctx *ctx, const hb_u128 *node_ids, uint64_t n);
/* Drops the batches appended since the last hb_finalize (device chunks, endpoint table, host buffer): the stream starts
 * empty again.  For callers that find out mid-stream that their source is damaged (hb_load_webgraph on a CRC mismatch). */
int hb_discard_appended(hb_ctx *ctx);

/* HB_FLAG_REFERENCE_TAIL only; after the graph is loaded, before hb_begin / hb_run.  records = the store's page-level
 * (from_id, to_id, rel_flags) documents, SEGMENT BY SEGMENT IN DOC ORDER (sort_score ascending, store.rs:67-72) - the
 * order decides what `graph.search(ForwardlinksQuery::new(h).with_limit(Unlimited))` returns (harmonic.rs:82-87): the
 * query runs one LinksScorer per segment over the documents whose from_id is h, which skips self links and every
 * document whose to_id equals the to_id of the document it yielded LAST (adjacent de-duplication, plus a skip-list
 * shortcut over whole 128-document blocks; query/raw/links.rs:115-232) BEFORE harmonic.rs:87 looks at the flags of
 * what is left.  So of two neighbouring documents (h -> x) with different flags only the first one's flags count.
 * The library replays exactly that per segment and host, then applies the rel filter (:87) and the two counter
 * lookups (:91-92).  Any superset of the relevant documents may be passed (documents whose from_id is no host node
 * are dropped at once); hb_tail_segment_end() marks the end of a segment, hb_begin closes the last one.
 * hb_load_tail_edges replaces the records of earlier calls (one segment, or the first part of one); count == 0 =
 * "the query finds nothing" (also the state before the first call). */
int hb_load_tail_edges(hb_ctx *ctx, const hb_edge *records, uint64_t count);
/* The same in batches (a crawl's page-level documents do not fit one array): a batch continues the current segment;
 * 24 bytes per document whose from_id is a host node stay on the host until the segment ends, 8 bytes per surviving
 * record after.  The index is built and uploaded by the next hb_begin / hb_run. */
int hb_append_tail_edges(hb_ctx *ctx, const hb_edge *records, uint64_t count);
/* The documents appended since the last call (or since hb_load_tail_edges) were one whole segment. */
int hb_tail_segment_end(hb_ctx *ctx);

/* Pre-reduced input (bench / large synthetic graphs): sorted_ids strictly ascending;
 * in-edges of node v (the v-th smallest id) are src[row_ptr[v] .. row_ptr[v+1]), already
 * unique and flag-filtered.  In edge-partition mode: full id list, local edge subset. */
int hb_load_dense(hb_ctx *ctx, const hb_u128 *sorted_ids, uint64_t n, const uint64_t *row_ptr,
                  const uint32_t *src, uint64_t m_eff);

/* ---- compute ----------------------------------------------------------------------------- */
/* Replaces calculate_centrality (harmonic.rs:215-287): runs passes until one changes
 * nothing, then normalises.  Blocking.  stats may be NULL. */
int hb_run(hb_ctx *ctx, hb_stats *stats);

/* Step-wise form of the same loop (parity tests, multi-rank drivers):
 *   hb_begin        initialize (harmonic.rs:53-73,219-235): counters, Kahan sums, t = 0
 *   hb_step         one loop body (harmonic.rs:237-280); *has_changes as in the reference
 *   hb_finish       normalize_centralities (harmonic.rs:178-195, :282)
 * hb_run == hb_begin; while (has_changes) hb_step; hb_finish. */
int hb_begin(hb_ctx *ctx);
int hb_step(hb_ctx *ctx, int *has_changes);
int hb_finish(hb_ctx *ctx);

int hb_get_stats(const hb_ctx *ctx, hb_stats *out);
/* Stats of pass t (0 <= t < passes). */
int hb_get_pass_stats(const hb_ctx *ctx, uint64_t t, hb_pass_stats *out);

/* ---- results: HarmonicCentrality::iter / len (harmonic.rs:296-311) ---------------------- */
/* Number of nodes with centrality > 0 (absent key <=> centrality <= 0). */
int hb_result_count(hb_ctx *ctx, uint64_t *count);
/* Ascending NodeID, only centrality > 0, value = sum / (n-1) (non-finite -> 0.0).
 * Writes min(count, cap) entries; ids or vals may be NULL. */
int hb_result_copy(hb_ctx *ctx, hb_u128 *ids, double *vals, uint64_t cap);

/* The second half of store_harmonic (centrality/mod.rs:92-103): ranks[j] = position of the j-th result
 * (hb_result_copy order) when all results are sorted by (Reverse(f64::total_cmp(centrality)), NodeID
 * ascending) - the value written to the "harmonic_rank" store.  Computed on the GPU (stable radix sort).
 * cap must be >= hb_result_count. */
int hb_result_ranks(hb_ctx *ctx, uint64_t *ranks, uint64_t cap);

/* top_nodes(&store, TopNodes::Top(k)) (centrality/mod.rs:33-52), which build_harmonic calls with k = 1_000_000 for
 * harmonic.csv (entrypoint/centrality.rs:55-68): the min(k, count) results with the largest centrality, descending
 * (f64::total_cmp); ties in ascending NodeID = the first k of the harmonic_rank order.  (The reference's sorted_k is an
 * unstable sort keyed by the centrality alone: the order of ties, and which of them make the cut, are unspecified
 * there.)  ids or vals may be NULL; *written = number of entries. */
int hb_result_top(hb_ctx *ctx, uint64_t k, hb_u128 *ids, double *vals, uint64_t *written);

/* ---- sampled page-level harmonic centrality: ApproxHarmonic::build (approx_harmonic.rs:40-89) ------------------------------------ */
/* k sources, one BFS each to distance max_dist + 1 (dijkstra_multi returns when it POPS a cost above max_dist, so nodes at max_dist + 1
 * are already in its map: shortest_path.rs:85-95), all run at once as bit sets over the device plan, 512 sources per batch.  Single
 * rank only.  Definitions (deterministic; the reference sums f32 terms from rayon threads):
 *   c_d(v)   = number of sources at distance exactly d from v, d = 1 .. max_dist + 1 (a source itself, d = 0, never counts: :63)
 *   norm     = (float)N / ((float)k_req * ((float)N - 1.0f))       (:57; N = num_nodes, k_req = requested samples)
 *   w_d      = (1.0f / (float)d) * norm                             (:69, f32)
 *   value(v) = (double)(float)S(v),  S(v) = sum over d ascending with c_d(v) > 0 of (double)c_d(v) * (double)w_d, from +0.0 in f64
 * v is a result iff some c_d(v) > 0.  The result replaces the context's results (hb_result_*, hb_store_harmonic_results) until the next
 * hb_begin / hb_run; the HyperBall state is not part of it (hb_run afterwards computes what it computed before).
 * Sampler (sources == NULL): candidates = the nodes with >= 1 out-edge in the loaded graph (self links included), ascending NodeID
 * (`page_edges().map(from).unique()`); min(k, candidates) distinct indices by Floyd's algorithm driven by splitmix64(seed) (index
 * j = next() % (i + 1)), sorted ascending.  Source i of the sorted list is bit i % 512 of batch i / 512. */
#define HB_SAMPLE_MAX_LEVELS 16
typedef struct hb_sample_options {
    uint32_t struct_size;   /* = sizeof(hb_sample_options); 0 = this version                                            */
    uint32_t max_dist;      /* 0 = 7 (approx_harmonic.rs:62); <= 15, else HB_ERR_LIMIT                                   */
    uint64_t seed;          /* sampler seed                                                                               */
    uint64_t samples;       /* k_req; 0 = ceil(log2((double)N) / (epsilon * epsilon)) (0 for N <= 1), or source_count
                               when sources are given; <= 65535, else HB_ERR_LIMIT                                        */
    uint64_t num_nodes;     /* N; 0 = the loaded graph's n                                                                */
    double   epsilon;       /* 0 = 0.3 (approx_harmonic.rs:29)                                                            */
    const hb_u128 *sources; /* NULL = seeded sampler; else source_count distinct node ids of the loaded graph              */
    uint64_t source_count;
} hb_sample_options;

typedef struct hb_sample_stats {
    uint32_t struct_size;   /* = sizeof(hb_sample_stats); 0 = this version                                               */
    uint32_t levels;        /* D = max_dist + 1                                                                           */
    uint64_t k_req;         /* requested samples (norm uses it)                                                           */
    uint64_t sources;       /* sources used                                                                               */
    uint64_t batches;       /* ceil(sources / 512)                                                                        */
    uint64_t results;       /* nodes with a value                                                                         */
    double   ms_total;      /* wall time of the call                                                                      */
    uint64_t level_changed[HB_SAMPLE_MAX_LEVELS]; /* node rows whose set grew at level d + 1, summed over the batches      */
    uint32_t level_modes[HB_SAMPLE_MAX_LEVELS];   /* bit m set = some batch ran level d + 1 in mode m (0 dense, 1 bitmap,
                                                     2 sweep; the A_t rule of hb_run); 0 = never run (every batch ended)  */
    double   level_ms[HB_SAMPLE_MAX_LEVELS];      /* GPU time of level d + 1, summed over the batches                     */
} hb_sample_stats;

int hb_sampled_harmonic(hb_ctx *ctx, const hb_sample_options *opt, hb_sample_stats *stats);
/* The sampler alone: the sorted sources hb_sampled_harmonic would use for (seed, k); *written = min(k, candidates).  out needs
 * min(k, candidates) entries (may be NULL to ask for the count). */
int hb_sample_sources(hb_ctx *ctx, uint64_t seed, uint64_t k, hb_u128 *out, uint64_t *written);
/* c_d(v) of the last hb_sampled_harmonic: out[v * D + d - 1], v in ascending NodeID order (n x D entries, D = stats.levels). */
int hb_debug_sample_histogram(hb_ctx *ctx, uint16_t *out);

/* ---- exact shortest-path distances: ShortestPaths (webgraph/shortest_path.rs:26-227) ---------------------------------------------- */
/* dijkstra_multi (shortest_path.rs:57-103) with unit edge costs = one breadth-first search from a set of sources, over the loaded
 * graph (host- or page-level; HB_FLAG_ALL_RELS contexts = the ShortestPaths trait, default contexts = the AMPC shortest-path job,
 * which drops SKIPPED_REL edges).  Every source has distance 0, an edge adds 1, and a u8 holds the distance: a node is only inserted
 * while cost + 1 < 255, so the largest distance reported is 254 and everything further is absent.  With HB_DIST_WITH_MAX the nodes at
 * distance <= max_dist are expanded (the reference returns when it POPS a larger cost), so distances up to min(max_dist + 1, 254) are
 * reported.  HB_DIST_REVERSED follows the edges backwards: the distance from every node TO the nearest source.  A source id that is not
 * a node of the graph contributes nothing and is counted in unknown_sources; duplicates count once.
 * Level-synchronous and direction-optimising (top-down / bottom-up steps); single rank only.  The call keeps its
 * result in buffers of its own: hb_result_* of an earlier hb_run / hb_sampled_harmonic stay as they are, a later hb_run computes what it
 * computed before, and the distances stay readable until the next hb_distances or the next load.  Refused (HB_ERR_INVALID) between
 * hb_begin and hb_finish, without a loaded graph, with world_size > 1, with source_count == 0 and with both debug flags set. */
#define HB_DIST_REVERSED        0x1u  /* follow edges backwards: distance from every node TO the source set (raw_reversed_distances*) */
#define HB_DIST_WITH_MAX        0x2u  /* max_dist is meaningful (raw_*_with_max); without it the walk runs to exhaustion */
#define HB_DIST_TOP_DOWN_ONLY   0x4u  /* debug: never switch to the bottom-up step (same result) */
#define HB_DIST_BOTTOM_UP_ONLY  0x8u  /* debug: bottom-up from level 1 on (same result) */
#define HB_DIST_UNREACHED       255u

typedef struct hb_distance_options {
    uint32_t struct_size, flags;                    /* struct_size = sizeof(hb_distance_options); 0 = this version; flags = HB_DIST_* */
    uint32_t max_dist;                              /* 0..255, as the reference's u8 */
    const hb_u128 *sources; uint64_t source_count;  /* dijkstra_multi takes a slice: >= 1 ids */
} hb_distance_options;

typedef struct hb_distance_stats {
    uint32_t struct_size;       /* = sizeof(hb_distance_stats); 0 = this version */
    uint32_t levels;            /* levels run */
    uint32_t max_distance;      /* largest distance found */
    uint64_t reached;           /* nodes with a distance, sources included */
    uint64_t unknown_sources;   /* ids not in the loaded graph */
    uint64_t edges_inspected;   /* src / reader entries actually read */
    uint64_t frontier[256];     /* nodes first reached at each level */
    uint8_t  step[256];         /* per level: 0 = top-down, 1 = bottom-up */
    double   ms_total, ms_levels; /* wall time of the call / GPU time of the level loop */
} hb_distance_stats;

int hb_distances(hb_ctx *ctx, const hb_distance_options *opt, hb_distance_stats *stats);
/* The result of the last hb_distances.  count = reached nodes; copy = those nodes only, ascending NodeID (the reference's
 * BTreeMap<NodeID, u8>), at most cap entries, ids or dist may be NULL; all = one byte per node in ascending-NodeID order (the order of
 * hb_result_copy's ids and hb_debug_copy_graph), HB_DIST_UNREACHED = no distance, cap >= n. */
int hb_distance_count(hb_ctx *ctx, uint64_t *count);
int hb_distance_copy(hb_ctx *ctx, hb_u128 *ids, uint8_t *dist, uint64_t cap);
int hb_distance_all(hb_ctx *ctx, uint8_t *dist, uint64_t cap);

/* ---- exact betweenness centrality: Betweenness (webgraph/centrality/betweenness.rs:29-172) ------------------------------------------ */
/* Brandes' algorithm ("A Faster Algorithm for Betweenness Centrality") from a set of source nodes over the loaded graph (host- or
 * page-level).  The loaded graph is already reduced to unique edges, and a self link never lies on a shortest path, so the
 * ForwardlinksQuery's skip_self_links / de-duplication (betweenness.rs:73-75) need nothing extra here.
 * Sources: given as ids; duplicates count once, ids that are no node of the graph are counted in unknown_sources.  sources == NULL means
 * every node when n <= 100000 (.take(100_000), betweenness.rs:34), HB_ERR_INVALID otherwise: the reference takes an arbitrary 100 000
 * from a hash set, which nothing can reproduce.  S = the distinct known sources, in ascending NodeID order; source i is lane i % 8 of
 * batch i / 8.
 * Per source s (betweenness.rs:50-122):
 *   dist_s(v)  = BFS distance, a u8, 255 = unreached;
 *   sigma_s(v) = number of shortest s -> v paths, a u64 with SATURATING add (order-independent for non-negative terms, ~0 absorbing);
 *   delta_s(v) = sum over the out-neighbours w with dist_s(w) == dist_s(v) + 1 of (sigma_s(v) / sigma_s(w)) * (1 + delta_s(w)), in f64
 *                from +0.0 (:104-115), computed in the algebraic form sigma_s(v) * sum((1 + delta_s(w)) / sigma_s(w)), without FMA
 *                contraction and without floating-point atomics.  The order of the terms of one (s, v) is not pinned by the reference
 *                (hash-set and document order decide it there); here the device layout fixes it: two calls give the same bits.
 * Result (:118-140): sum(v) = delta_s(v) over the sources s != v in ascending order; value(v) = sum(v) / (S * (S - 1)), one f64
 * division, so S == 1 gives 0 / 0 = NaN and x / 0 = +inf, as the reference does.  HB_BC_RAW returns sum(v) itself: a caller may split
 * its sources over several calls and add.  v is a result iff it is a source or some source reaches it (:56, :119).
 * Limits: a walk that still has a frontier after level 254, and any sigma that saturates (the reference's i32 would have wrapped at
 * 2^31), end the call with HB_ERR_LIMIT and leave NO result: a truncated betweenness would be a wrong one.
 * Single rank only.  The result lives in buffers of its own until the next hb_betweenness or the next load; hb_result_* of an earlier
 * run and the last hb_distances result stay readable.  The walk borrows the HyperBall state (registers, partials, changed bitmaps,
 * sweep scratch) as hb_sampled_harmonic does: hb_step needs a new hb_begin afterwards, and a later hb_run computes what it computed
 * before.  Refused (HB_ERR_INVALID) between hb_begin and hb_finish, without a loaded graph, with world_size > 1, with both debug flags
 * set and with sources == NULL on a graph of more than 100000 nodes.  DESIGN.md section 15. */
#define HB_BC_RAW          0x1u  /* the result is sum(v), not sum(v) / (S (S - 1)) */
#define HB_BC_DENSE_ONLY   0x2u  /* debug: every forward level is a dense one (same result) */
#define HB_BC_SPARSE_ONLY  0x4u  /* debug: every forward level is a sweep (bitmap on a context without sweep support; same result) */

typedef struct hb_betweenness_options {
    uint32_t struct_size, flags;                    /* struct_size = sizeof(hb_betweenness_options); 0 = this version; flags = HB_BC_* */
    const hb_u128 *sources; uint64_t source_count;  /* NULL = every node (n <= 100000) */
} hb_betweenness_options;

typedef struct hb_betweenness_stats {
    uint32_t struct_size;       /* = sizeof(hb_betweenness_stats); 0 = this version */
    uint32_t max_dist;          /* largest distance over all sources (Betweenness::max_dist) */
    uint64_t sources;           /* S: distinct known sources */
    uint64_t unknown_sources;   /* ids not in the loaded graph */
    uint64_t batches;           /* ceil(S / 8) */
    uint64_t results;           /* sources and nodes reached from one */
    uint64_t levels_forward, levels_backward; /* levels run, over all batches */
    uint64_t levels_mode[3];    /* forward levels per mode: dense, bitmap, sweep */
    uint64_t edges_gathered;    /* source entries gathered by the forward levels */
    uint64_t device_bytes;      /* the operator's own buffers */
    double   ms_total;          /* wall time of the call */
    double   ms_forward, ms_backward; /* GPU time of the forward / backward levels */
    double   ms_mode[3];        /* GPU time of the forward levels per mode */
    double   ms_dense_max;      /* the slowest dense forward level */
} hb_betweenness_stats;

int hb_betweenness(hb_ctx *ctx, const hb_betweenness_options *opt, hb_betweenness_stats *stats);
/* The result of the last hb_betweenness.  count = results; copy = those nodes only, ascending NodeID, at most cap entries, ids or vals
 * may be NULL (only the results are downloaded); all = one f64 per node in ascending-NodeID order, -1.0 = no result, cap >= n. */
int hb_betweenness_count(hb_ctx *ctx, uint64_t *count);
int hb_betweenness_copy(hb_ctx *ctx, hb_u128 *ids, double *vals, uint64_t cap);
int hb_betweenness_all(hb_ctx *ctx, double *vals, uint64_t cap);
/* Debug: the per-lane state of the LAST batch of the last hb_betweenness, n x 8 entries each in ascending-NodeID order (entry sid * 8 +
 * lane; lanes beyond the batch's sources: 255 / 0 / +0.0); any of the three may be NULL. */
int hb_debug_copy_betweenness_batch(hb_ctx *ctx, uint8_t *dist, uint64_t *sigma, double *delta);

/* ---- inbound similarity: Scorer (ranking/inbound_similarity.rs:61-138) over BitVec (ranking/bitvec_similarity.rs:131-189) ---------- */
/* The score of EVERY node of the loaded graph against a list of liked and a list of disliked hosts (searcher/api/mod.rs:199-216,
 * similar_hosts.rs).  in(v) = the in-neighbours of v in the loaded graph.
 * BitVec of a node (bitvec_similarity.rs:144-163): len = |in(v)|, sqrt_len = sqrt(len as f64), and a bloom of 16 u64 words in which the
 * low id word x of every in-neighbour sets bit (x * 11400714819323198549 mod 2^64) % 64 of word (the same product) % 16; ones = bits set.
 * Both indices come from one product and 16 divides 64, so the bloom is kept as ONE u64 mask (bit h & 63): same ones, same intersections.
 * sim(a, v) (:165-180) = 0.0 if either len is 0; 0.0 if popcount(bloom_a & bloom_v) / max(ones_a, ones_v) < 0.25 (tested as
 * 4 * intersect_ones < max_ones in integers: the quotient of two integers <= 1024 is never within an ulp of 0.25); else
 * |in(a) & in(v)| as f64 / (sqrt_len_a * sqrt_len_v) - one multiply, one division, no FMA contraction.
 * score(v) (Scorer::calculate_score, inbound_similarity.rs:99-118) = max(0.0, s) with s = D + (sum_liked - sum_disliked), divided by
 * max(L, 1) with HB_SIM_NORMALIZED; L / D = the number of liked / disliked entries; both sums run in entry order from +0.0; an entry
 * whose id is v contributes self_score (1.0 unless HB_SIM_SELF_SCORE) instead of sim.  Duplicate entries each count.  An entry that is
 * no node of the graph has an empty BitVec: its sim is 0, it counts in L or D (and in hb_similarity_stats.unknown).
 * Defined differences: the relation filter of the load applies (HB_SKIPPED_REL_MASK drops NOFOLLOW among others; HB_FLAG_ALL_RELS keeps
 * everything), edges are unique, and in(v) depends on hb_similarity_options.limit:
 *   limit == 0: in(v) is the WHOLE in-list of the loaded graph, self links as loaded.  The reference takes EdgeLimit::Limit(512) backlinks
 *     in search order before it filters: the two agree wherever every host involved has at most 512 inbound records and no self link.
 *   1 <= limit <= 1024 (the reference's Scorer: 512, searcher/api/mod.rs:199-216 batch_raw_ingoing_hosts(nodes, EdgeLimit::Limit(512))):
 *     in(v) = backlinks(v, limit) as hb_backlinks below defines it under the CURRENT key set (hb_links_set_keys; none: NodeID order) - the
 *     in-neighbours u != v (LinksQuery.skip_self_links), ordered by (key[u], NodeID u) ascending, the first min(limit, degree(v)) of them.
 *     This holds for EVERY node, anchors included: len = min(degree(v), limit), the bloom covers THOSE entries only, the intersection is
 *     |inL(a) & inL(v)|.  What differs from the reference is then what differs for hb_backlinks: the limit best of the whole list instead
 *     of the first limit + 128 documents, unsaturated keys, the load's relation filter.  hb_inbound_similarity(limit = 512) +
 *     hb_similarity_top give that score for ALL hosts, without the <= 1024-candidate pre-selection of hb_similar_hosts.
 *     A node row is LISTED when its cut differs from its list as loaded (degree > limit, or a self link); only listed rows get an explicit
 *     cut list (limit x 4 bytes each, plus one u32 per node row), built at the first limited call and kept while graph, key set and limit
 *     stay the same: hb_links_set_keys, a call with another limit > 0 and the next load drop it.  limit > 1024 is refused
 *     (HB_ERR_INVALID) before the previous result is touched.
 * Entry 16 b + j (liked entries first, then the disliked ones, in caller order) is slot j of batch b; a batch is one level of the walk
 * the other operators share (hb_sampled_harmonic, hb_betweenness) with sixteen u32 counts per 64-byte row and a plain add as the join.
 * Single rank only.  The call borrows the HyperBall state as those walks do: hb_step needs a new hb_begin afterwards, a later hb_run
 * computes what it computed before, the results of hb_run / hb_distances / hb_betweenness stay readable.  The per-graph state (one
 * position byte, one in-degree and one u64 bloom per row) is built at the first call after a load and freed by the next load; the
 * scores live in buffers of their own until the next hb_inbound_similarity or the next load.  Refused (HB_ERR_INVALID) between hb_begin
 * and hb_finish, without a loaded graph, with world_size > 1, with both debug flags set and with no entry at all.  DESIGN.md section 16. */
#define HB_SIM_NORMALIZED   0x1u  /* Scorer::new(.., normalized = true): s / max(L, 1) */
#define HB_SIM_DENSE_ONLY   0x2u  /* debug: every count level is a dense one (same result) */
#define HB_SIM_SPARSE_ONLY  0x4u  /* debug: every count level is a sweep (bitmap on a context without sweep support; same result) */
#define HB_SIM_SELF_SCORE   0x8u  /* Scorer::set_self_score(self_score); without it self_score = 1.0 */
#define HB_SIM_TOP_SKIP_ANCHORS 0x1u /* hb_similarity_top: leave the liked / disliked hosts out (similar_hosts.rs:163) */

typedef struct hb_similarity_options {
    uint32_t struct_size, flags;                    /* struct_size = sizeof(hb_similarity_options); 0 = this version; flags = HB_SIM_* */
    const hb_u128 *liked;    uint64_t liked_count;
    const hb_u128 *disliked; uint64_t disliked_count;
    double self_score;                              /* used only with HB_SIM_SELF_SCORE */
    uint32_t limit, reserved;                       /* 0 = whole in-lists (also what a caller with the shorter struct_size gets); 1 .. 1024 =
                                                     * every BitVec from backlinks(v, limit); the reference's Scorer uses 512 */
} hb_similarity_options;

typedef struct hb_similarity_stats {
    uint32_t struct_size;       /* = sizeof(hb_similarity_stats); 0 = this version */
    uint32_t reserved;
    uint64_t liked, disliked;   /* L, D: entries as given (duplicates and unknown ids included) */
    uint64_t unknown;           /* entries that are no node of the graph */
    uint64_t batches;           /* ceil((L + D) / 16) */
    uint64_t rows_nonzero;      /* node rows with a non-zero count, summed over the batches */
    uint64_t levels_mode[3];    /* count levels per mode: dense, bitmap, sweep (a batch without a known anchor runs none) */
    uint64_t edges_gathered;    /* source entries gathered by the count levels */
    uint64_t device_bytes;      /* the operator's own buffers */
    double   ms_total;          /* wall time of the call */
    double   ms_bloom;          /* GPU time of the per-graph state (0 when it existed) */
    double   ms_count;          /* GPU time of the count levels; with a limit also of the list-count kernel: sum(ms_mode) + ms_list_count */
    double   ms_score;          /* GPU time of seed + accumulate + score */
    double   ms_mode[3];        /* GPU time of the count levels per mode (the walk alone: ms_list_count is in none of them) */
    uint64_t listed_rows;       /* limited mode: node rows that hold an explicit cut list (0 with limit == 0) */
    uint64_t list_entries;      /* ... the entries of those lists */
    double   ms_lists;          /* ... GPU time of building them (0 when they existed) */
    double   ms_list_count;     /* ... GPU time of the list-count kernel over the batches: part of ms_count, of no ms_mode entry */
} hb_similarity_stats;

int hb_inbound_similarity(hb_ctx *ctx, const hb_similarity_options *opt, hb_similarity_stats *stats);
/* The result of the last hb_inbound_similarity.  all = one f64 per node in ascending-NodeID order, cap >= n.  lookup = Scorer::score of
 * the given hosts; an id that is no node of the graph gets the score of an empty BitVec (its only possible terms are the self_score of
 * the entries equal to it).  top = the first min(k, candidates) nodes in the order of sorted_k(Reverse((SortableFloat(score), node)))
 * (similar_hosts.rs:182-191): score descending, ties by NodeID descending; selection and sort run on the device, only those entries are
 * downloaded; ids or vals may be NULL; flags = HB_SIM_TOP_*. */
int hb_similarity_all(hb_ctx *ctx, double *vals, uint64_t cap);
int hb_similarity_lookup(hb_ctx *ctx, const hb_u128 *ids, uint64_t count, double *vals);
int hb_similarity_top(hb_ctx *ctx, uint64_t k, uint32_t flags, hb_u128 *ids, double *vals, uint64_t *written);
/* Debug: the counts of the LAST batch of the last hb_inbound_similarity (n x 16, entry sid * 16 + slot: |in(v) & in(anchor)|; slots
 * without a known anchor are 0), and the per-graph bloom masks and in-degrees (n each), ascending-NodeID order; any of the three may be
 * NULL.  The counts lie in the borrowed HyperBall state: refused once another call has used that state.  After a limited call the three
 * are the limited ones (|inL(v) & inL(anchor)|, the bloom over the cut entries, min(degree, limit)): refused once hb_links_set_keys has
 * dropped the cut lists. */
int hb_debug_copy_similarity_batch(hb_ctx *ctx, uint32_t *counts, uint64_t *bloom, uint32_t *len);

/* ---- nearest-seed centrality: HarmonicNearestSeed (entrypoint/centrality.rs:126-201, `stract centrality harmonic-nearest-seed`) ------ */
/* Completes a centrality that covers only some nodes (ApproxHarmonic: hb_sampled_harmonic): for EVERY node v of the loaded graph
 * (stream_page_node_ids, entrypoint/webgraph.rs:113-160) - if the original centrality has a value for v, v gets it unchanged
 * (centrality.rs:153-156; Some(0.0) is a value); otherwise v gets original(seed(v)) * discount_factor, one f64 multiply (:158-176,
 * default discount_factor 0.5: config/defaults.rs:230), and nothing when v has no seed or the seed has no value - there is no fallback
 * to a second backlink.
 * seed(v) = the `from` of the first result of BacklinksQuery::new(v).with_limit(Limit(1)) (query/backlink.rs:96-209): the in-neighbour
 * u != v of v (self links are skipped, LinksQuery.skip_self_links, query/raw/links.rs:31-49,194) that minimises (key[u], NodeID u), where
 * key is the caller's per-node order key - the harmonic rank of the node's host, which is what sort_score = from_host_rank
 * .saturating_add(to_host_rank) orders one node's backlinks by (ascending: query/collector/top_docs.rs:394-400, query/document_scorer/
 * mod.rs).  A node that is not in the key list has key u64::MAX, which is an ordinary key: a node whose only in-neighbour is unlisted
 * still has that seed.  seed(v) is defined for every node, those with an original value included; none if v has no in-neighbour other
 * than itself.
 * Defined differences (each is something the reference leaves to chance): ties in the key go to the smaller NodeID; keys are compared
 * unsaturated, which is the reference's order whenever from_rank + to_rank < 2^64 (with a destination rank of u64::MAX every backlink
 * ties there); the in-list is that of the loaded graph, whatever relation filter the load applied - the reference applies none, so load
 * with HB_FLAG_ALL_RELS; edges are unique in the loaded graph (the reference de-duplicates by `from`).
 * Rounds: val_0 = the original values.  Round r = 1 .. rounds: a node without a value after round r - 1 whose seed has one gets
 * val_(r-1)(seed) * discount_factor; synchronous (the state after r - 1 is read, the state after r written), one multiply per hop.
 * rounds = 1 (or 0) is the reference; more rounds follow the chain of best-rank backlinks further (an extension).  The loop stops after
 * the first round that fills nothing.
 * The orig list is the original_centrality Db: duplicate ids - the last one wins (Db::insert); ids that are no node of the graph are
 * ignored and counted; a NaN or a value with its sign bit set is refused (HB_ERR_INVALID).  Presence is a flag of its own, not val > 0.
 * HB_SEED_FROM_IMAGE: the original is the context's live result (hb_run / hb_sampled_harmonic, as hb_result_copy lists it), read on the
 * device; refused without one.
 * Single rank only.  The operator borrows nothing: hb_run / hb_step, hb_result_*, hb_distances, hb_betweenness and
 * hb_inbound_similarity results are untouched, and its own result lives in buffers of its own until the next successful
 * hb_nearest_seed or the next load - a refused call leaves it as it was.  Refused (HB_ERR_INVALID) between hb_begin and hb_finish,
 * without a loaded graph, with world_size > 1, with opt == NULL, a discount_factor that is not finite or negative, rounds > 255,
 * HB_SEED_FROM_IMAGE together with an orig list, and an orig or key pointer NULL with a non-zero count.  DESIGN.md section 19. */
#define HB_SEED_FROM_IMAGE 0x1u  /* original = the context's live result (hb_run / hb_sampled_harmonic); orig_* must be NULL / 0 */

typedef struct hb_nearest_seed_options {
    uint32_t struct_size, flags;                    /* struct_size = sizeof(hb_nearest_seed_options); 0 = this version; flags = HB_SEED_* */
    double   discount_factor;                       /* finite, >= 0; no default: 0.0 means 0.0 */
    uint32_t rounds;                                /* 0 = 1 = the reference; at most 255 */
    uint32_t reserved;
    const hb_u128 *orig_ids; const double *orig_vals; uint64_t orig_count;  /* the original_centrality Db */
    const hb_u128 *key_ids;  const uint64_t *keys;    uint64_t key_count;   /* per-node order key (the host's harmonic rank); a node not
                                                                                listed has u64::MAX; NULL / 0 = none */
} hb_nearest_seed_options;

typedef struct hb_nearest_seed_stats {
    uint32_t struct_size;         /* = sizeof(hb_nearest_seed_stats); 0 = this version */
    uint32_t rounds_run;          /* rounds executed (the first one that fills nothing is the last) */
    uint64_t with_original;       /* nodes with an original value */
    uint64_t filled[16];          /* nodes filled by round 1, 2, ...; rounds beyond the 16th are summed into the last entry */
    uint64_t unknown_orig;        /* entries of the orig list that are no node of the graph */
    uint64_t unknown_keys;        /* entries of the key list that are no node of the graph */
    uint64_t no_seed;             /* nodes that end without a value and have no seed */
    uint64_t seed_without_value;  /* nodes that end without a value although they have a seed */
    uint64_t results;             /* nodes with a value: with_original + the sum of filled[] */
    uint64_t device_bytes;        /* the operator's own buffers */
    double   ms_total;            /* wall time of the call */
    double   ms_seed;             /* GPU time of the seed level (candidates, chunk rows, node rows) */
    double   ms_fill;             /* GPU time of round 0, the rounds and the result in NodeID order */
} hb_nearest_seed_stats;

int hb_nearest_seed(hb_ctx *ctx, const hb_nearest_seed_options *opt, hb_nearest_seed_stats *stats);
/* The result of the last hb_nearest_seed.  count = results; copy = those nodes only, ascending NodeID, at most cap entries, ids or vals
 * may be NULL (only the results are downloaded); all = one f64 per node in ascending-NodeID order, -1.0 = no result, cap >= n; top =
 * the first min(k, results) rows of harmonic.csv (centrality.rs:186-195): value descending, ties by NodeID ASCENDING (hb_similarity_top
 * breaks ties the other way), selected and sorted on the device, only those pairs are downloaded; seeds = seed(v) of EVERY node in
 * ascending-NodeID order, has_seed[v] = 0 (and a zero id) where there is none, cap >= n, either array may be NULL. */
int hb_nearest_seed_count(hb_ctx *ctx, uint64_t *count);
int hb_nearest_seed_copy(hb_ctx *ctx, hb_u128 *ids, double *vals, uint64_t cap);
int hb_nearest_seed_all(hb_ctx *ctx, double *vals, uint64_t cap);
int hb_nearest_seed_top(hb_ctx *ctx, uint64_t k, hb_u128 *ids, double *vals, uint64_t *written);
int hb_nearest_seed_seeds(hb_ctx *ctx, hb_u128 *seed, uint8_t *has_seed, uint64_t cap);

/* ---- limited, rank-ordered host backlinks: HostBacklinksQuery::new(v).with_limit(EdgeLimit::Limit(L)) (query/backlink.rs:230-360) ---- */
/* The link query the reference's callers reach the graph with (inbound_similarity::Scorer: L = 512 per liked / disliked host;
 * SimilarHostsFinder::potential_nodes, similar_hosts.rs:118-165: L = 128; harmonic_nearest_seed: L = 1; RemoteWebgraph::batch_search
 * sends them by the thousand), for a LIST of hosts per call.
 * in(v) = the in-neighbours u != v of v in the loaded graph: edges are unique, the load applied its relation filter, a self link is
 * skipped as LinksQuery.skip_self_links does (HB_LINKS_KEEP_SELF keeps it).  key[u] = a u64 per node, u64::MAX for a node that is not
 * listed, as in the reference.  Order: (key[u], NodeID u) ascending - sids ascend with the NodeIDs, so (key, sid); the order
 * hb_nearest_seed defined.  backlinks(v, L) = the first min(L, |in(v)|) elements of in(v) in that order, LISTED in that order;
 * degree(v) = |in(v)|, what HostGroupQuery::backlinks(v, ToHostId, FromHostId) counts.  hb_nearest_seed's seed(v) is backlinks(v, 1).
 * Defined differences: the reference stops collecting after L + 128 documents in document order and de-duplicates hosts afterwards -
 * here the list is the L best of the WHOLE in-list; sort_score saturates in the reference, keys are compared unsaturated (as
 * hb_nearest_seed); the query's text and rel filters are not supported, the load's relation mask is the filter (load with
 * HB_FLAG_ALL_RELS for the reference's unfiltered list); EdgeLimit::Unlimited and LimitAndOffset are not offered.
 * hb_links_set_keys: the key set, either as a list (key_ids, keys, key_count: a duplicate id - the last one wins; an id that is no node
 * is counted in unknown_keys) or HB_LINKS_KEYS_FROM_RANKS: key = the rank hb_result_ranks reports for the live result (hb_run /
 * hb_sampled_harmonic), u64::MAX for a node without a result; refused without a live result and together with a list.  The call builds,
 * on the device and once per key set, the dense order ord[sid] = the position of the node in the sort by (key, sid), its inverse and ord
 * by device row.  Keys and order stay on the device until the next hb_links_set_keys or the next load.  Without any call every key is
 * u64::MAX: the order is NodeID order.
 * hb_backlinks: the lists of `nodes` with 1 <= limit <= 1024.  An id that is no node of the graph gets an empty list and degree 0 (and
 * is counted in unknown); the same id may be given several times, each occurrence gets the full answer.  slots_per_batch = how many
 * distinct hosts one batch of the device loop holds (0 = 1024; at most 65536).  Device memory is O(n_pad + nv + slots x (256 + limit))
 * besides the result (queries x limit): it does not grow with the in-degrees of the queried hosts, and the work is proportional to the
 * lists of the queried hosts.  The result is deterministic.
 * Single rank only.  The operator borrows nothing: hb_run / hb_step, hb_result_*, hb_distances, hb_betweenness, hb_inbound_similarity
 * and hb_nearest_seed results are untouched; its buffers are its own, allocated at first use after a load, freed by the next load and
 * counted in device_bytes.  The result lives until the next successful hb_backlinks / hb_forwardlinks or the next load - a refused call
 * leaves it as it was.  Both calls are refused (HB_ERR_INVALID) between hb_begin and hb_finish, without a loaded graph and with world_size > 1;
 * hb_links_set_keys also with a key pointer NULL and a non-zero count; hb_backlinks also with opt == NULL, limit 0 or above 1024,
 * slots_per_batch above 65536 and nodes == NULL with a non-zero node_count.  DESIGN.md section 27. */
#define HB_LINKS_KEYS_FROM_RANKS 0x1u /* hb_links_set_keys: key = harmonic rank of the live result; key_* must be NULL / 0 */
#define HB_LINKS_KEEP_SELF    0x1u  /* hb_backlinks: a self link is an entry like any other */
#define HB_LINKS_SPREAD_ORDS  0x2u  /* debug: the select runs on ord * floor(2^32 / n) (strictly monotone: same result; all four digits) */
#define HB_LINKS_NO_SHORTCUT  0x4u  /* debug: lists with degree <= limit go through the select too (same result) */

typedef struct hb_links_key_options {
    uint32_t struct_size, flags;                    /* struct_size = sizeof(hb_links_key_options); 0 = this version; flags = HB_LINKS_KEYS_* */
    const hb_u128 *key_ids; const uint64_t *keys; uint64_t key_count;
} hb_links_key_options;

typedef struct hb_links_key_stats {
    uint32_t struct_size;         /* = sizeof(hb_links_key_stats); 0 = this version */
    uint32_t reserved;
    uint64_t listed;              /* nodes with a key of their own */
    uint64_t unknown_keys;        /* entries of the key list that are no node of the graph */
    uint64_t device_bytes;        /* the operator's own buffers */
    double   ms_total;            /* wall time of the call */
    double   ms_order;            /* GPU time of the sort and of ord / inverse / ord by row */
} hb_links_key_stats;

typedef struct hb_links_options {
    uint32_t struct_size, flags;                    /* struct_size = sizeof(hb_links_options); 0 = this version; flags = HB_LINKS_* */
    const hb_u128 *nodes; uint64_t node_count;      /* the queried hosts, in the order hb_links_copy answers in */
    uint32_t limit;                                 /* L: 1 .. 1024 */
    uint32_t slots_per_batch;                       /* 0 = 1024 */
} hb_links_options;

typedef struct hb_links_stats {
    uint32_t struct_size;         /* = sizeof(hb_links_stats); 0 = this version */
    uint32_t reserved;
    uint64_t queries;             /* node_count */
    uint64_t unknown;             /* queries that are no node of the graph */
    uint64_t distinct;            /* distinct nodes among the others (each is looked up once) */
    uint64_t batches;
    uint64_t entries;             /* entries of all lists, as hb_links_copy returns them */
    uint64_t rows_walked;         /* node and chunk rows scanned by the expansion */
    uint64_t edges_gathered;      /* source entries counted by the expansion: the sum of degree(v) over the distinct nodes */
    uint64_t selected;            /* distinct nodes whose list went through the radix select */
    uint64_t device_bytes;        /* the operator's own buffers */
    double   ms_total;            /* wall time of the call */
    double   ms_expand;           /* GPU time of expansion and count */
    double   ms_select;           /* GPU time of the select rounds */
    double   ms_emit;             /* GPU time of emit, sort and translation */
} hb_links_stats;

int hb_links_set_keys(hb_ctx *ctx, const hb_links_key_options *opt, hb_links_key_stats *stats);
int hb_backlinks(hb_ctx *ctx, const hb_links_options *opt, hb_links_stats *stats);
/* ---- limited, rank-ordered host forward links: HostForwardlinksQuery::new(u).with_limit(EdgeLimit::Limit(L)) (query/forwardlink.rs:183-330) ----
 * The mirror of hb_backlinks, what SimilarHostsFinder::potential_nodes (similar_hosts.rs:118-165) sends with L = 512 from the sources of
 * the liked hosts' backlinks.  out(u) = the out-neighbours v != u of u in the loaded graph (HB_LINKS_KEEP_SELF keeps a self link);
 * order: (key[v], NodeID v) ascending - for a fixed source the reference's sort_score = source_rank + destination_rank orders by the
 * destination's rank, so this is the order hb_links_set_keys built; forwardlinks(u, L) = the first min(L, |out(u)|) elements of out(u)
 * in that order, listed in that order; degree(u) = |out(u)|.  The same options struct, limit range, batch knob, debug flags, refusals and
 * defined differences as hb_backlinks (the L best of the WHOLE out-list, no L + 128 document short-circuit; keys unsaturated; no text
 * or rel filters, no Unlimited, no offset).  In the stats rows_walked counts the pieces of 2048 reader-list entries the batches scanned,
 * edges_gathered the sum of degree(u) over the distinct nodes.
 * The first call after a load builds, besides the holders hb_backlinks has, a table of 4 x virtual_rows bytes (the node row on top of
 * every hub-chunk row: an out-edge into a hub enters its chunk tree at some chunk row) and, in a context without sweep support
 * (HB_FLAG_NO_SPARSE, unfused passes), the row -> readers transpose that hb_distances builds; it refuses with "unexpected plan layout"
 * when a chunk row does not have exactly one reader.  Device memory is O(n_pad + nv + slots x (256 + limit)) besides the result: it does
 * not grow with the out-degrees.  The result is deterministic and replaces that of the last hb_backlinks / hb_forwardlinks:
 * hb_links_count / hb_links_copy read the last successful call of either direction.  DESIGN.md section 28. */
int hb_forwardlinks(hb_ctx *ctx, const hb_links_options *opt, hb_links_stats *stats);
/* The result of the last hb_backlinks / hb_forwardlinks.  count: its queries and the entries of all lists.  copy: offsets[i] .. offsets[i + 1] is the list
 * of query i (caller order; queries + 1 offsets), ids / keys the entries in list order (at most cap of them: cap >= entries),
 * degrees[i] = degree(v_i); any of the four may be NULL, only what is asked for is downloaded. */
int hb_links_count(hb_ctx *ctx, uint64_t *queries, uint64_t *entries);
int hb_links_copy(hb_ctx *ctx, uint64_t *offsets, uint64_t *degrees, hb_u128 *ids, uint64_t *keys, uint64_t cap);

/* ---- similar hosts: scored_nodes of SimilarHostsFinder::find_similar_hosts (similar_hosts.rs:54-272) for a list of liked hosts ---- */
/* Input: nodes[0 .. N) and limit k.  N counts the entries as given: a duplicate counts twice in the score and in N, an id that is no node
 * contributes nothing but counts in N.  With backlinks / forwardlinks as defined above, under the current key set:
 *  1. In512(a) = backlinks(a, 512) of every distinct liked host; its first 128 entries are backlinks(a, 128) (similar_hosts.rs:118-131).
 *  2. B = the distinct sources in those 128-prefixes, nb = |B|.
 *  3. forwardlinks(b, 512) of every b in B (:133-143).
 *  4. count[v] = the number of those lists that contain v.  apply = nb > 32; with apply only count[v] <= ceil(0.25 nb) stay - the bound
 *     is computed in integers as (nb + 3) / 4 (:145-151); the rest ordered by (count descending, NodeID ascending) - the reference's tie
 *     order is hash-map iteration order, this one is the defined difference -; the first (apply ? 256 : 1024) are taken; only THEN are
 *     the liked hosts dropped (:152-164, in that order: a liked host inside the prefix leaves the list one short).
 *  5. BitVec of a candidate c = backlinks(c, 512): len = min(degree, 512), the entries sorted, the 64-bit bloom mask of
 *     hb_inbound_similarity (bit (low64(id) x 11400714819323198549) & 63) over THOSE entries only (searcher/api/mod.rs:199-216,
 *     ranking/bitvec_similarity.rs:131-180).
 *  6. score[c] = max(0, (sum over the entries a in caller order, from 0.0, of sim(a, c)) / max(N, 1)) - Scorer::new(liked, [],
 *     normalized = true).  sim = 0 when 4 popcount(mask_a & mask_c) < max(popcount mask_a, popcount mask_c) (integers) or a list is
 *     empty, else |In512(a) & In512(c)| / (sqrt((double)len_a) x sqrt((double)len_c)): IEEE sqrt, one multiply, one divide, no FMA
 *     contraction, no floating-point atomics.
 *  7. the first min(k, candidates) by (score descending, NodeID descending): sorted_k over Reverse((SortableFloat, NodeID)), the tie
 *     rule of hb_similarity_top.
 * The reference's dead-link pass (:228-237) is not built: on one consistent graph it is vacuous - a candidate was reached over an edge
 * from some b != c, so its in-degree is at least 1.  Names, root_domain and the `limit + len + 30` arithmetic stay with the caller
 * (stract_amd/similar_hosts.py does them in Python).  The steps run on the device; sizes and the two final lists (at most 1024 entries
 * each) come to the host.  hb_similar_candidates returns the pre-selection of step 4 after the liked hosts are dropped, in its order,
 * with the counts.  flags: HB_LINKS_SPREAD_ORDS / HB_LINKS_NO_SHORTCUT reach the list selects (debug: same result).
 * The operator borrows nothing, leaves the result of the last hb_backlinks / hb_forwardlinks readable (its lists go to buffers of its
 * own, counted in device_bytes), and its result lives until the next successful call or the next load; a refused call changes nothing.
 * Refused (HB_ERR_INVALID): opt == NULL, node_count == 0, nodes == NULL, more than 256 distinct known nodes, limit outside 1 .. 1024,
 * between hb_begin and hb_finish, without a loaded graph, world_size > 1.  DESIGN.md section 28. */
typedef struct hb_similar_options {
    uint32_t struct_size, flags;                    /* struct_size = sizeof(hb_similar_options); 0 = this version */
    const hb_u128 *nodes; uint64_t node_count;      /* the liked hosts, in the order the score sums them */
    uint32_t limit, reserved;                       /* k: 1 .. 1024 */
} hb_similar_options;

typedef struct hb_similar_stats {
    uint32_t struct_size;         /* = sizeof(hb_similar_stats); 0 = this version */
    uint32_t apply;               /* 1 = the popularity filter was on (nb > 32) */
    uint64_t liked_distinct;      /* distinct known liked hosts */
    uint64_t unknown;             /* entries that are no node of the graph */
    uint64_t nb;                  /* |B| */
    uint64_t forward_entries;     /* entries of the forward lists of B */
    uint64_t distinct_targets;    /* nodes with count > 0 */
    uint64_t count_bound;         /* (nb + 3) / 4 */
    uint64_t taken;               /* entries taken in step 4 before the liked hosts are dropped */
    uint64_t candidates;          /* ... after */
    uint64_t pairs_gated;         /* (candidate, entry) pairs the bloom gate set to 0 */
    uint64_t pairs_intersected;   /* ... whose lists were intersected */
    uint64_t written;             /* min(k, candidates) */
    uint64_t device_bytes;        /* the operator's own buffers */
    double   ms_total;            /* wall time of the call */
    double   ms_in, ms_forward, ms_count, ms_bitvec, ms_score;   /* wall time per stage: steps 1-2, 3, 4, 5, 6-7 */
    double   ms_gpu_lists, ms_gpu_score;                         /* GPU time of the list selects; of score + top */
} hb_similar_stats;

int hb_similar_hosts(hb_ctx *ctx, const hb_similar_options *opt, hb_similar_stats *stats);
int hb_similar_count(hb_ctx *ctx, uint64_t *count);
int hb_similar_copy(hb_ctx *ctx, hb_u128 *ids, double *scores, uint64_t cap);   /* the top list, at most cap >= count entries */
int hb_similar_candidates(hb_ctx *ctx, hb_u128 *ids, uint64_t *counts, uint64_t cap, uint64_t *written); /* ids / counts may be NULL */

/* ---- scoring result hosts: inbound_similarity::Scorer::score per search, as the InboundScorer stage calls it ------------------------ */
/* What the searcher does with a query that carries host rankings (searcher/api/mod.rs:467-501: Scorer::new(webgraph, liked, disliked,
 * false); :411-465 combine_results and :199-216 batch_raw_ingoing_hosts: the BitVec of every unique result host from
 * EdgeLimit::Limit(512) backlinks; ranking/pipeline/scorers/inbound_similarity.rs:38-54: Scorer::score(host, inbound) for at most 300
 * pages) - for several searches per call, with work proportional to (result hosts + anchors) x limit instead of the graph.
 * Everything holds under the current key set of hb_links_set_keys.
 * BitVec(v) for 1 <= limit <= 1024 is exactly the BitVec of hb_inbound_similarity with that limit: the entries are backlinks(v, limit),
 * sorted; len = min(degree(v), limit); the 64-bit bloom mask covers those entries only; an id that is no node of the graph has the
 * empty BitVec.
 * A request is (liked[], disliked[], nodes[], flags, self_score).  For every entry v of nodes, in caller order:
 *   score(v) = max(0.0, s) with s = D + (sum_liked - sum_disliked), in exactly that grouping; with HB_SIM_NORMALIZED s is divided by
 *   max(L, 1).  L and D count the liked and disliked entries as given: duplicates and unknown ids count.  Each sum runs in caller order
 *   from +0.0.
 * A pair (anchor a, node v) is classified in this order:
 *   1. self: the NodeIDs are equal, also for ids that are no node; it contributes self_score (1.0 unless HB_SIM_SELF_SCORE).
 *   2. empty: either len is 0; it contributes 0.0.
 *   3. gated: 4 popcount(ma & mv) < max(popcount(ma), popcount(mv)), in integers; it contributes 0.0.
 *   4. intersected: it contributes |inL(a) & inL(v)| as f64 / (sqrt(len_a) x sqrt(len_v)) - IEEE sqrt, one multiply and one divide, no
 *      FMA contraction, no floating-point atomics.
 * This is NodeScorer::sim + BitVec::sim + Scorer::calculate_score (ranking/inbound_similarity.rs:44-50,99-118).
 * The contract: for every request the result is bit for bit what hb_inbound_similarity(the same liked, disliked, flags, self_score,
 * limit) followed by hb_similarity_lookup(nodes) returns on the same context and key set.
 * The operator borrows nothing (no HyperBall rows, no result image), leaves the results of every other operator readable - the links,
 * similar-hosts and similarity results included -, keeps holders of its own in the graph state (they only grow, are counted in
 * device_bytes and freed by the next load: O(distinct x limit) plus one piece of the pair space plus the entries of the call), and its
 * result lives until the next successful call or the next load; a refused call changes nothing.  A request without nodes yields an
 * empty slice, one without anchors scores of max(0, 0).
 * Refused (HB_ERR_INVALID): opt == NULL, request_count == 0 or above 4096, a NULL pointer with a non-zero count, limit outside 1 .. 1024,
 * slots_per_batch > 65536, more than 2^24 anchor plus node entries in total, more than 262144 distinct known hosts, between hb_begin and
 * hb_finish, without a loaded graph, world_size > 1, an unexpected plan layout.  DESIGN.md section 30. */
#define HB_SCORE_SMALL_PIECES 0x100u /* debug: the pair space is walked in pieces of 64 pairs instead of 2^20 (same result) */

typedef struct hb_score_request {
    const hb_u128 *liked;    uint64_t liked_count;
    const hb_u128 *disliked; uint64_t disliked_count;
    const hb_u128 *nodes;    uint64_t node_count;   /* the result hosts, scored in this order; duplicates each get the answer */
    uint32_t flags, reserved;                       /* HB_SIM_NORMALIZED | HB_SIM_SELF_SCORE */
    double self_score;                              /* used only with HB_SIM_SELF_SCORE */
} hb_score_request;

typedef struct hb_score_options {
    uint32_t struct_size, flags;                    /* struct_size = sizeof(hb_score_options); 0 = this version; flags: HB_LINKS_SPREAD_ORDS /
                                                       HB_LINKS_NO_SHORTCUT reach the list selects, HB_SCORE_SMALL_PIECES (debug: same result) */
    const hb_score_request *requests; uint64_t request_count;
    uint32_t limit, slots_per_batch;                /* 1 .. 1024 (the reference: 512); 0 = the list builder's default */
} hb_score_options;

typedef struct hb_score_stats {
    uint32_t struct_size, reserved; /* struct_size = sizeof(hb_score_stats); 0 = this version */
    uint64_t requests;
    uint64_t anchors, nodes;                   /* liked + disliked entries / node entries of all requests, as given */
    uint64_t unknown_anchors, unknown_nodes;   /* ... of which no node of the graph */
    uint64_t distinct;                         /* the known hosts of the call, each looked up once across all requests */
    uint64_t pairs;                            /* sum over the requests of nodes x anchors = the four classes below */
    uint64_t pairs_self, pairs_empty, pairs_gated, pairs_intersected;
    uint64_t pieces;                           /* launches of the pair kernel's piece loop */
    uint64_t device_bytes;                     /* the operator's own buffers */
    double   ms_total;                         /* wall time of the call */
    double   ms_lists, ms_bitvec, ms_pairs, ms_finish; /* GPU time: the list selects, the BitVec kernel, the pair kernel, the finish kernel */
} hb_score_stats;

int hb_score_hosts(hb_ctx *ctx, const hb_score_options *opt, hb_score_stats *stats);
/* The result of the last hb_score_hosts: offsets[r] .. offsets[r + 1] is the slice of request r (requests + 1 offsets), scores[] one f64
 * per node entry in caller order (cap >= the scores of hb_score_count); either may be NULL. */
int hb_score_count(hb_ctx *ctx, uint64_t *requests, uint64_t *scores);
int hb_score_copy(hb_ctx *ctx, uint64_t *offsets /* requests + 1 */, double *scores, uint64_t cap);

/* ---- multi-GPU (one process per GPU, RCCL over xGMI) -------------------------------------- */
/* Rank 0 calls this and distributes the 128 bytes (e.g. torch.distributed broadcast);
 * every rank puts them in hb_options.rccl_id. */
int hb_rccl_unique_id(uint8_t out[128]);

/* The exchanges of a pass through the CALLER's collectives instead of RCCL [r4]: a context created with world_size > 1 and
 * HB_FLAG_NO_RCCL behaves exactly like one with a communicator (same kernels, same row slices, same event ordering of the
 * merge / all-reduce / epilogue pipeline, same changed-only packing) once these three functions are set - every
 * ncclAllReduce / ncclAllGather / ncclBroadcast of the pass driver goes through them.  Purpose: (1) the multi-process
 * protocol can run as real library code on ONE device, N processes exchanging through host-staged torch.distributed
 * (gloo) tensors - tests/test_gpu.py, since RCCL refuses two ranks on one device; (2) an integrator whose ranks are
 * already connected by another fabric (MPI, the reference's own DHT) needs no RCCL bootstrap.
 * All pointers are DEVICE pointers; `stream` is the hipStream_t the call is ordered on (work queued on it before the call
 * must be visible to the exchange, work queued after it must see the result; a blocking implementation simply
 * synchronises the stream first).  Return 0, or non-zero to fail the pass with HB_ERR_RCCL.  Set before loading the graph. */
#define HB_COLL_U8 0
#define HB_COLL_U32 1
#define HB_COLL_U64 2
#define HB_COLL_F64 3
#define HB_COLL_MAX 0
#define HB_COLL_SUM 1
typedef struct hb_collectives {
    void *user;
    /* in place over `count` elements of `dtype` on every rank */
    int (*all_reduce)(void *user, void *buf, uint64_t count, int dtype, int op, void *stream);
    /* recv = world x bytes_per_rank bytes, rank r's part at r x bytes_per_rank; send may be that very part of recv */
    int (*all_gather)(void *user, const void *send, void *recv, uint64_t bytes_per_rank, void *stream);
    /* `bytes` bytes at buf from rank `root` to every rank */
    int (*broadcast)(void *user, void *buf, uint64_t bytes, int root, void *stream);
} hb_collectives;
int hb_set_collectives(hb_ctx *ctx, const hb_collectives *ops);
/* The one collective hb_collectives lacks, for HB_FLAG_PACKED_WIRE on the edge partition: piece k of `send`
 * (world x bytes_per_rank bytes) goes to rank k, piece k of `recv` comes from rank k; send != recv.  `user` is the pointer of
 * hb_set_collectives; device pointers and `stream` as for the other three.  Set after hb_set_collectives (which also clears it) and
 * before the graph is loaded; NULL removes it.  hb_begin refuses (HB_ERR_INVALID) on an edge-partitioned context that has
 * HB_FLAG_PACKED_WIRE and caller collectives but not this one.  A context with a communicator does the exchange itself. */
int hb_set_all_to_all(hb_ctx *ctx, int (*all_to_all)(void *user, const void *send, void *recv, uint64_t bytes_per_rank, void *stream));
/* helper for host-staged implementations of the above: copy on `stream`, then synchronise it (to_device: host -> device) */
int hb_debug_staged_copy(void *dst, const void *src, uint64_t bytes, int to_device, void *stream);

/* ---- pinned batch buffers ------------------------------------------------------------------- */
/* Page-locked host memory for the record batches of hb_append_edges / hb_load_edges (hipHostMalloc): a batch that lies
 * in pinned memory crosses the host link asynchronously at its full rate (57 GB/s measured on the MI355X boxes,
 * profiles/r04a_h2d_probe.txt) and overlaps with the reduction of the batch before it; from pageable memory the
 * runtime has to stage it.  A caller that owns its buffer can pin it in place with hipHostRegister instead.
 * hb_pinned_free(NULL) is a no-op. */
int hb_pinned_alloc(uint64_t bytes, void **out);
void hb_pinned_free(void *p);

/* ---- device helpers for harnesses -------------------------------------------------------- */
int hb_device_count(int *count);
/* Fills name (NUL-terminated, <= cap) with the gcnArchName of the ctx device. */
int hb_device_name(const hb_ctx *ctx, char *name, uint64_t cap);
int hb_device_synchronize(hb_ctx *ctx);

/* ---- test / bench-only exports (NOT part of the drop-in contract) ------------------------- */
/* Current counters, one 64-byte register block per node, in ascending-NodeID order
 * (HyperLogLog::registers, hyperloglog.rs:4544).  Valid after hb_begin / any hb_step. */
int hb_debug_copy_registers(hb_ctx *ctx, uint8_t *out /* n*64 */);
/* KahanSum state per node, ascending-NodeID order (kahan_sum.rs:30-33). */
int hb_debug_copy_kahan(hb_ctx *ctx, double *sum, double *err);
/* Cached HyperLogLog::size() of the current counter per node. */
int hb_debug_copy_sizes(hb_ctx *ctx, uint64_t *out);
/* Runs the device estimator (HyperLogLog::size, hyperloglog.rs:4484-4516) on `count`
 * arbitrary 64-byte register blocks. */
int hb_debug_hll_size(hb_ctx *ctx, const uint8_t *regs, uint64_t count, uint64_t *out);
/* Order-independent 64-bit checksums of the current state: out[0] over all counters, out[1] over the
 * Kahan (sum, err) bit patterns; node v (v-th smallest NodeID) contributes a mix of (v, its words), summed
 * mod 2^64 (definition: oracle/hb_oracle.c hbo_dense_state_hash computes the same function).  For per-pass
 * parity at sizes where n*64 bytes are too many to ship.  Multi-rank contexts: out[1] = 0 (a rank holds the
 * Kahan state of its own rows only); out[0] covers all counters (every rank holds them after the collective). */
int hb_debug_state_hash(hb_ctx *ctx, uint64_t out[2]);
/* Reduced graph as the library sees it after ingest (ascending-NodeID indexing):
 * any pointer may be NULL; row_ptr has n+1 entries, src has m_eff.  row_ptr / src are kept on the host only for
 * graphs of up to 2^26 edges, or with HB_FLAG_HOST_PLAN (HB_ERR_LIMIT otherwise). */
int hb_debug_copy_graph(hb_ctx *ctx, hb_u128 *ids, uint64_t *row_ptr, uint32_t *src);
/* The device work layout of the loaded graph as it lies in HBM (same conventions as hb_host_plan: two-call
 * pattern, sizes = {n_pad, nv, plan_src_len, levels}; order[n_pad], plan_row_ptr[n_pad+nv+1], plan_src[plan_src_len],
 * level_begin[levels+1]).  The device planner must reproduce the host planner's layout entry for entry. */
int hb_debug_copy_plan(hb_ctx *ctx, uint64_t sizes[4], uint32_t *order, uint64_t *plan_row_ptr, uint32_t *plan_src,
                       uint64_t *level_begin);
/* The live-first part of the loaded graph's layout (HB_FLAG_LIVE_FIRST): live = {1 if the order is in use else 0, n_live = hosts with
 * >= 1 in-edge (device rows [0, n_live) when the order is in use), n_live_pad = the end of the node-row launches of passes t >= 1
 * (n_live rounded up to 64 with the order, n_pad without)}. */
int hb_debug_plan_live(hb_ctx *ctx, uint64_t live[3]);
/* The saturated rows of the run in progress (HB_FLAG_NO_SATURATION): info = {1 if the context skips saturated rows else 0, n, nv,
 * the work rows (node rows and hub chunks) of the last dense pass that left their gather loop early, 1 if that pass ran the early-exit
 * instances else 0 (HB_FLAG_NO_EARLY_EXIT; a pass that did not counts nothing)};
 * u[64] = U, the register-wise maximum of the initial counters of the hosts with an out-link; node_bits[n] = 1 where the host's row
 * (input order, like hb_debug_copy_registers) is marked saturated; virt_bits[nv] = the same for the hub-chunk rows in the order of
 * hb_debug_copy_plan.  Pointers may be NULL; a context that does not skip reports info[0] = 0 and writes nothing else. */
int hb_debug_saturation(hb_ctx *ctx, uint64_t info[5], uint8_t *u, uint8_t *node_bits, uint8_t *virt_bits);
/* Emulates the collective of one pass between `count` logical ranks that live on ONE device
 * (contexts created with HB_FLAG_NO_RCCL; RCCL refuses two ranks on one device).
 *   phase 0, between hb_step_local and hb_step_finish of every context:
 *     edge partition:        all-reduce(max) of the pending counters
 *     destination partition: all-gather of the owned counter / changed-bit slices, sum of the
 *                            changed counts (ctxs[i] must be rank i)
 *     HB_FLAG_PACKED_WIRE contexts: the packed forms of these, device copies in place of the collectives
 *   phase 1, before hb_finish: all-gather of the Kahan-sum slices. */
int hb_debug_exchange(hb_ctx **ctxs, int count, int phase);
/* The three kernels of HB_FLAG_PACKED_WIRE on arbitrary rows (unit-test and measurement door): rows = pieces x count x 64 host bytes
 * (piece k = rows [k count, (k + 1) count)) are uploaded, packed to 48-byte rows, the register-wise maximum over the pieces is taken
 * in packed form and unpacked.  packed_max = count x 48 bytes, rows_out = count x 64 bytes (either may be NULL); ms = the GPU time
 * of the pack of all pieces, of the maximum and of the unpack, by events on the context's stream.  rows == NULL: every piece is the
 * context's own resident counters (count <= the padded row count of the loaded graph, after hb_begin), nothing is uploaded. */
int hb_debug_wire6(hb_ctx *ctx, const uint8_t *rows, uint64_t count, uint32_t pieces, uint8_t *packed_max, uint8_t *rows_out, float ms[3]);
/* Two halves of hb_step: local pull into the pending counters; [collective, or hb_debug_exchange];
 * then (edge partition / HB_FLAG_UNFUSED) estimator/Kahan/changed detection, bookkeeping. */
int hb_step_local(hb_ctx *ctx);
int hb_step_finish(hb_ctx *ctx, int *has_changes);

/* Bench hook: the rate (GB/s) at which `bytes` bytes at `host` reach the device through hipMemcpyAsync on the library's stream,
 * mean of `reps` copies into a scratch buffer - what hb_append_edges can get from this buffer in this process. */
int hb_debug_h2d_rate(hb_ctx *ctx, const void *host, uint64_t bytes, int reps, double *gb_per_s);
/* Test hook: lowers the limits of the device ingest so that its refusal (>= max_records -> host ingest), its
 * out-of-memory spill (chunk memory beyond max_device_bytes counts as a failed allocation) and its multi-chunk
 * paths (chunk_records per chunk) can be reached with small inputs.  0 = default for each. */
int hb_debug_set_ingest_limits(hb_ctx *ctx, uint64_t max_records, uint64_t max_device_bytes, uint64_t chunk_records);

/* ---- host-only test exports (no device needed) -------------------------------------------- */
/* The reference ingest semantics alone (node set, first-occurrence de-duplication, flag
 * filter; store.rs:297-357, harmonic.rs:131).  Two-call pattern: with ids/row_ptr/src NULL
 * only the counts are returned; then row_ptr needs n+1 and src m_eff entries. */
int hb_host_ingest(const hb_u128 *node_ids, uint64_t n, const hb_edge *edges, uint64_t m,
                   uint64_t *n_out, uint64_t *m_unique, uint64_t *m_eff, hb_u128 *ids,
                   uint64_t *row_ptr, uint32_t *src);
/* The device work layout the planner would build for a reduced graph (device order +
 * hub-row splitting), so its invariants can be checked on the host.  flags: HB_FLAG_NO_REORDER, HB_FLAG_NO_XCD_MAP.
 * Two-call pattern: sizes[0..3] = {n_pad, nv, plan_src_len, levels}; then
 * order[n_pad] (0xFFFFFFFF = padding row), plan_row_ptr[n_pad+nv+1], plan_src[plan_src_len],
 * level_begin[levels+1].  tune[7] > 1 lays the rows out as tune[7] owner slices (destination partition). */
int hb_host_plan(uint64_t n, const uint64_t *row_ptr, const uint32_t *src, uint32_t flags,
                 uint32_t chunk, const uint32_t *tune /* hb_options.tune or NULL */, uint64_t sizes[4],
                 uint32_t *order, uint64_t *plan_row_ptr, uint32_t *plan_src, uint64_t *level_begin);
/* The live-first order (HB_FLAG_LIVE_FIRST) is planned under the rule of a single-rank context with these `flags` and this n: one
 * slice, a reordered plan, no flag that makes the passes unfused or counting; on from 2^20 nodes, HB_FLAG_LIVE_FIRST /
 * HB_FLAG_NO_LIVE_FIRST force it on / off.  hb_host_plan_live: what hb_debug_plan_live reports, for that plan. */
int hb_host_plan_live(uint64_t n, const uint64_t *row_ptr, const uint32_t *src, uint32_t flags, uint32_t chunk, const uint32_t *tune,
                      uint64_t live[3]);
/* Host only (no GPU): the index hb_load_tail_edges / hb_append_tail_edges build from page-level records (taken as ONE
 * segment in doc order) - CSR by SOURCE device row (dev_of[sid]) over the records the per-host LinksScorer yields that
 * pass the rel filter and whose two ids are nodes (harmonic.rs:87,91-92), duplicates dropped.  ptr_out: n_pad + 1 offsets; to_out: target device rows (first to_cap), *to_len = their number. */
int hb_debug_tail_index(uint64_t n, const hb_u128 *sorted_ids, const uint32_t *dev_of, uint64_t n_pad, const hb_edge *records,
                        uint64_t count, uint64_t *ptr_out, uint32_t *to_out, uint64_t to_cap, uint64_t *to_len);

#ifdef __cplusplus
}
#endif
#endif /* HYPERBALL_H */
