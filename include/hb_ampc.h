/*
 * hb_ampc.h - a GPU-resident shard of the AMPC table store: what the harmonic-centrality and the shortest-path job of the
 * reference's distributed variant keep per shard.
 *
 * The harmonic job keeps `counters: DefaultDhtTable<NodeID, HyperLogLog<64>>` and `centrality: DefaultDhtTable<NodeID, KahanSum>`
 * (crates/core/src/entrypoint/ampc/harmonic_centrality/mod.rs:47-53), the shortest-path job `distances: DefaultDhtTable<NodeID, u64>`
 * (shortest_path/mod.rs:51-55), in a raft-replicated key-value store driven by batch operations (harmonic_centrality/mapper.rs:52-209,
 * shortest_path/mapper.rs:57-103):
 *     batch_set     setup_counters, update_centralities                  dht/store.rs (insert / overwrite)
 *     batch_get     get_old_counters, get_old_distances
 *     batch_upsert  update_counters (`HyperLogLog64Upsert`), update_distances (`U64Min`)   dht/upsert.rs, dht/store.rs:159-190
 *     clone_table   init_from at the start of every round                dht/store.rs:192-195, ampc/dht_conn.rs:271-277
 * batch_upsert applies the pairs IN ORDER: an absent key is inserted (`Inserted`, the pair's value verbatim); otherwise
 * merged = op(old, new) and the action is `Merged` iff merged != old (Rust's derived PartialEq: an IEEE comparison for the float kinds,
 * so a NaN result is always `Merged` and -0.0 turning into +0.0 is `NoChange` although the merged bits are stored), else `NoChange`.
 * This header is the C ABI a GPU worker would put behind those calls.  A table lives in HBM: the key -> slot index is a device hash
 * table (hb_table.hip.h), the values one array of 64 / 8 / 4 / 8 / 16 / 64 bytes each.  A batch is grouped by key with its order kept and
 * every group is folded by one writer in that order (HyperLogLog: one quad per key; the scalar kinds: one thread per key, one wave for
 * a key with many pairs).  hbu_update_centralities is CentralityMapper::update_centralities (mapper.rs:157-209) as one device call:
 * no counter and no size crosses the link.  The two steps that walk the EDGES are device calls between two resident tables as well:
 *     hbu_update_counters   CentralityMapper::update_counters (mapper.rs:89-111): batch_get of edge.from, add_u128(edge.from),
 *                           batch_upsert(HyperLogLog64Upsert) into edge.to - 32 B of ids up and one action byte back per edge
 *     hbu_update_distances  ShortestPathMapper::update_distances (shortest_path/mapper.rs:64-86): batch_get of edge.from, + 1, the
 *                           batch's own minimum per destination, batch_upsert(U64Min) - ids up, one (key, action) per destination back
 * so that clone -> edge step -> update_centralities -> swap is a whole round of either job with no counter on the link.
 * In: HyperLogLog<64> with HyperLogLog64Upsert; u64 with U64Add / U64Min; f32 with F32Add; f64 with F64Add; KahanSum with KahanSumAdd
 * (upsert.rs:92-152); the copy of a table; update_centralities; update_counters; update_distances; a worker's graph and its changed-node
 * filter (U64BloomFilter, the Exact arm of UpdatedNodes) resident next to the tables, with one call per mapper step (setup_counters,
 * map_cardinalities, RelaxEdges, map_centralities); what the approximated-harmonic coordinator (approximated_harmonic_centrality/
 * coordinator.rs:82-180) adds to the shortest-path job: the fold of a finished job's distances into the KahanSum table as one device call
 * (hbu_fold_harmonic), the worker's node sketch (hbu_graph_node_sketch, HyperLogLog<4096> registers) and DhtTable::iter() for a table of any
 * kind (hbu_export); and the step that job needs to run at a useful speed, several sampled sources per walk over the edges: a sixth table
 * kind whose 64-byte row holds one u8 distance for each of up to 64 sources (HBU_KIND_DIST64, HBU_OP_DIST64_MIN), RelaxEdges for all of
 * them in one pass (hbu_round_lane_distances) and their fold in source order (hbu_fold_harmonic_lanes).  The reference's max_distance is
 * a u8 (config/mod.rs:718), so a distance fits a lane; max_distance = 255 stays with the per-source route; and the finish of both jobs:
 * the stored value of every key of the centrality table (f64::from(c) / (num_nodes - 1) as f64, harmonic_centrality/coordinator.rs:204-211;
 * f64::from(*c), approximated_harmonic_centrality/coordinator.rs:152-157), store_harmonic and top_nodes (webgraph/centrality/mod.rs:33-114)
 * as three device calls (hbu_finish_centralities, hbu_top_centralities, hbu_store_centralities): only the results cross the link.
 * Still out: harmonic.csv (it needs node names), HyperLogLog<8/16/32/128> as table values (no job uses them), HyperLogLog<4096>::size() (its bias rows are
 * not carried here: the caller merges the registers and estimates), the sampling of sources, more than 64 lanes or 16-bit lanes, a lane
 * form of the host-fed edge step, the String, meta and
 * bloom-valued tables (a handful of values per shard), the Exact -> Sketch policy of UpdatedNodes and the serde envelopes of the filters
 * (the caller's), a compressed edge layout, raft replication, the network protocol, shards that span ranks.
 * Defined differences: U64Add wraps at 2^64 (the reference panics in a debug build and wraps in a release build), and so does the
 * `+ 1` of hbu_update_distances; an operator that does not belong to the table's kind is refused with HB_ERR_INVALID and changes
 * nothing (the reference panics); HBU_FOLD_SKIP_ZERO (off by default) keeps a sampled source's own distance 0 out of the fold.
 *
 * extern "C", never unwinds, 0 = ok, negative = HB_ERR_* of hyperball.h; needs a gfx950 device (no CPU fallback).
 */
#ifndef HB_AMPC_H
#define HB_AMPC_H

#include <stdint.h>

#include "hyperball.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hbu_table hbu_table;

#define HBU_NO_CHANGE 0 /* UpsertAction::NoChange  (dht/upsert.rs:24-28) */
#define HBU_MERGED    1 /* UpsertAction::Merged                          */
#define HBU_INSERTED  2 /* UpsertAction::Inserted                        */

#define HBU_KIND_HLL64 0 /* 64 B: HyperLogLog<64>::registers; what hbu_create makes */
#define HBU_KIND_U64   1 /*  8 B                                                    */
#define HBU_KIND_F32   2 /*  4 B                                                    */
#define HBU_KIND_F64   3 /*  8 B                                                    */
#define HBU_KIND_KAHAN 4 /* 16 B: {double sum, err}  (kahan_sum.rs:30-33)           */
#define HBU_KIND_DIST64 5 /* 64 B: 64 lanes of u8, one per source of a batch; HBU_DIST_NONE = no distance */

#define HBU_OP_HLL64     0 /* register-wise max                                      upsert.rs:67-89   */
#define HBU_OP_U64_ADD   1 /* old + new, wrapping                                    upsert.rs:92-103  */
#define HBU_OP_U64_MIN   2 /* min(old, new)                                          upsert.rs:105-116 */
#define HBU_OP_F32_ADD   3 /* old + new: one f32 addition per pair, in batch order   upsert.rs:118-129 */
#define HBU_OP_F64_ADD   4 /* old + new: one f64 addition per pair, in batch order   upsert.rs:131-142 */
#define HBU_OP_KAHAN_ADD 5 /* old += new.sum (kahan_sum.rs:47-54); new.err ignored   upsert.rs:143-152 */
#define HBU_OP_DIST64_MIN 6 /* byte-wise min: U64Min (upsert.rs:105-116) on each of a row's 64 lanes    */

#define HBU_DIST_LANES 64   /* lanes of an HBU_KIND_DIST64 row                                          */
#define HBU_DIST_NONE  0xFF /* a lane without a distance; lanes hold 0 .. 254                           */

/* device < 0: current device.  capacity_hint: expected number of keys (the table grows as needed). */
int hbu_create(int32_t device, uint64_t capacity_hint, hbu_table **out);
int hbu_create_kind(int32_t device, uint64_t capacity_hint, uint32_t kind, hbu_table **out);
int hbu_kind(const hbu_table *t, uint32_t *kind, uint32_t *value_bytes);
void hbu_destroy(hbu_table *t);
const char *hbu_last_error(const hbu_table *t);
int hbu_len(const hbu_table *t, uint64_t *keys);

/* counters: count x 64 bytes (HyperLogLog<64>::registers).  Later pairs of the same key win. */
int hbu_batch_set(hbu_table *t, const hb_u128 *keys, const uint8_t *counters, uint64_t count);
/* found[i] = 0 for an absent key (counters_out[i] is then all zero = HyperLogLog::default()). */
int hbu_batch_get(hbu_table *t, const hb_u128 *keys, uint64_t count, uint8_t *counters_out, uint8_t *found);
/* HyperLogLog64Upsert over the pairs in order; actions[i] = HBU_* for pair i. */
int hbu_batch_upsert(hbu_table *t, const hb_u128 *keys, const uint8_t *counters, uint64_t count, uint8_t *actions);


/* ---- any kind.  values: count x value_bytes, in the table's kind.  On an HBU_KIND_HLL64 table these are the three calls above (op =
 * HBU_OP_HLL64); the three calls above are refused (HB_ERR_INVALID, table untouched) on a table of another kind, and so is an
 * operator that does not belong to the table's kind. */
int hbu_batch_set_values(hbu_table *t, const hb_u128 *keys, const void *values, uint64_t count);
/* an absent key: found[i] = 0 and zero bytes (0 / 0.0 / KahanSum::default()); on an HBU_KIND_DIST64 table 64 bytes of HBU_DIST_NONE: "no
 * distance", not zero, is that kind's default.  HBU_OP_DIST64_MIN follows the rule above: an absent key is Inserted with the pair's row
 * verbatim (a row of 64 x HBU_DIST_NONE included), otherwise merged = byte-wise min(old, new), Merged iff merged != old.  The three counter
 * calls are refused on an HBU_KIND_DIST64 table although its rows are as wide. */
int hbu_batch_get_values(hbu_table *t, const hb_u128 *keys, uint64_t count, void *values_out, uint8_t *found);
int hbu_batch_upsert_values(hbu_table *t, uint32_t op, const hb_u128 *keys, const void *values, uint64_t count, uint8_t *actions);
/* pairs of one key up to this many are folded by one thread, more by one wave (tests place groups at this length) */
uint32_t hbu_wave_group_length(void);

/* clone_table: a new table of the same kind on the same device with the same keys and values; independent afterwards.
 * Device-to-device copies only. */
int hbu_clone(hbu_table *from, hbu_table **out);

/* DhtTable::iter(): every (key, value) of the table, any kind (hbu_create's counter tables included; values_out: len x value_bytes); the
 * entry with entry number p goes to position p, so keys_out[i] belongs to values_out[i]; the order is otherwise unspecified.  *written =
 * len.  capacity < len: HB_ERR_INVALID, nothing written.  An empty table: HB_OK, *written = 0, the two arrays may be NULL. */
int hbu_export(hbu_table *t, hb_u128 *keys_out, void *values_out, uint64_t capacity, uint64_t *written);

/* CentralityMapper::update_centralities (mapper.rs:157-209) for `count` nodes, all four tables on one device: a node found in BOTH
 * counter tables with d = next.size() saturating-minus prev.size() != 0 gets
 *     next_centrality[node] = (prev_centrality[node] or KahanSum::default()) + d as f64 / (round + 1) as f64
 * SET (not upserted; may insert the key).  *written = the number of distinct nodes set (a node listed twice counts once, as in the
 * reference's BTreeMap).  Refused with HB_ERR_INVALID: wrong kinds, tables on different devices, prev_centrality == next_centrality. */
int hbu_update_centralities(hbu_table *prev_counters, hbu_table *next_counters, hbu_table *prev_centrality, hbu_table *next_centrality,
                            const hb_u128 *nodes, uint64_t count, uint64_t round, uint64_t *written);

/* ---- the edge steps: `prev` is only read, `next` changes; both of one kind on one device.  Everything is visible on return (the call
 * runs on next's stream after a synchronise of prev's).  Refused with HB_ERR_INVALID, or HB_ERR_LIMIT for count >= 2^30 (checked before
 * an edge is read), both tables untouched and hbu_last_error set on next: NULL with a count, a wrong kind on either table, tables on
 * different devices, prev == next, a broken table.  count == 0: HB_OK, nothing touched.  Transactional like every batch call: after a
 * HIP error next holds the keys it held before. */

/* CentralityMapper::update_counters (mapper.rs:89-111) for `count` edges (from[i], to[i]), both tables HBU_KIND_HLL64: pair i =
 * (to[i], (prev[from[i]] or HyperLogLog::default() - unwrap_or_default, mapper.rs:98: an absent source is NOT a skipped edge) with
 * add_u128(from[i]): only the low 64 bits of from[i] are hashed, hyperloglog.rs:4398-4400, while the table key is all 128), upserted
 * into `next` with HyperLogLog64Upsert in edge order (an absent destination: Inserted, the pair's counter verbatim); actions[i] = HBU_*
 * of pair i.  Tables and actions equal, bit for bit, those of hbu_batch_get(prev, from) + add_u128 on the host +
 * hbu_batch_upsert(next, to, ...) for the same batch. */
int hbu_update_counters(hbu_table *prev_counters, hbu_table *next_counters, const hb_u128 *from, const hb_u128 *to, uint64_t count, uint8_t *actions);

/* ShortestPathMapper::update_distances (shortest_path/mapper.rs:64-86), both tables HBU_KIND_U64: an edge whose source has no distance
 * in `prev` is skipped (and inserts nothing: a destination all of whose edges were skipped is neither in the output nor in `next`); the
 * others give to[i] the candidate prev[from[i]] + 1 (2^64 - 1 wraps to 0); every distinct destination with a candidate is upserted ONCE
 * with U64Min and its smallest candidate: Inserted for an absent destination, Merged iff that candidate is below the stored value,
 * NoChange otherwise.  keys_out / actions_out (room for `count` entries each): one entry per such destination, *written of them, every
 * destination exactly once; their order is unspecified (the reference's is a hash map's iteration order), the set of entries is the
 * same for the same inputs. */
int hbu_update_distances(hbu_table *prev_distances, hbu_table *next_distances, const hb_u128 *from, const hb_u128 *to, uint64_t count,
                         hb_u128 *keys_out, uint8_t *actions_out, uint64_t *written);

#define HBU_FOLD_SKIP_ZERO 1u /* defined difference, off by default: entries with distance 0 (the source) are not folded */
/* approximated_harmonic_centrality/coordinator.rs:139-145 for one finished shortest-path job: for every (node, d) of `distances`
 * (HBU_KIND_U64), in one kernel of its own (the keys of a table are distinct: nothing is sorted or grouped),
 *     v = (1.0 / (double)d) * norm;   centralities[node] = absent ? KahanSum{v, 0.0} : centralities[node] += KahanSum{v, 0.0}
 * with AddAssign<KahanSum> as written (kahan_sum.rs:65-72: y = (v + 0.0) - err; t = sum + y; err = (t - sum) - y; sum = t), every
 * operation rounded on its own (no fused multiply-add).  `centralities` is HBU_KIND_KAHAN on the same device and may grow; `distances`
 * is only read.  *folded = the entries folded, *inserted = the new keys among them (either may be NULL).  The call runs on
 * centralities' stream after a synchronise of distances'; everything is visible on return.  Equal, bit for bit, to hbu_batch_get_values
 * of every key of `distances`, v on the host and hbu_batch_upsert_values(HBU_OP_KAHAN_ADD) for norm > 0.
 * `norm` is taken as given, inf included (the reference's num_samples == 1 gives 1.0 / 0).  A distance of 0 (the source itself) is
 * folded as the reference folds it: v = inf, so the first fold into a node stores {inf, 0 or NaN}, the next gives err = NaN, the one
 * after that sum = NaN: a sampled source ends up inf or NaN unless HBU_FOLD_SKIP_ZERO is set.  The sign and payload of a NaN are not
 * pinned (x86 and gfx950 produce different default NaNs for inf - inf).  2^64 - 1 and 2^53 + 1 convert as Rust's `as f64` does (round to
 * nearest even).  An empty `distances`: HB_OK, zero counts, nothing touched.  Refused with HB_ERR_INVALID, nothing changed, hbu_last_error
 * set on centralities: NULL, a wrong kind on either table, tables on different devices, a broken table, unknown flag bits.
 * Transactional like every batch call: after a HIP error `centralities` holds the keys it held before. */
int hbu_fold_harmonic(hbu_table *distances, hbu_table *centralities, double norm, uint32_t flags, uint64_t *folded, uint64_t *inserted);

/* hbu_fold_harmonic for a finished batch of up to 64 shortest-path jobs held as lane rows: for every key of `lanes` (HBU_KIND_DIST64) and
 * l = 0 .. n_lanes - 1 IN ASCENDING ORDER where byte l is not HBU_DIST_NONE, exactly what hbu_fold_harmonic does for (key, d = byte l) - the
 * first addend of a key absent from `centralities` written as {v, 0.0}, every other one added -, so that the result equals, bit for bit
 * except for a NaN's sign and payload, n_lanes calls of hbu_fold_harmonic, one per lane in lane order, on HBU_KIND_U64 tables holding that
 * lane's entries.  Lanes at or above n_lanes are ignored.  HBU_FOLD_SKIP_ZERO skips lanes that hold 0.  A key with no lane to fold is not
 * inserted and claims no entry.  *folded = the lanes folded, *inserted = the new keys (either may be NULL).  Room is made first for
 * committed + len(lanes) keys.  An empty `lanes`: HB_OK, zero counts, nothing touched.  Refused with HB_ERR_INVALID, nothing changed,
 * hbu_last_error set on centralities: n_lanes of 0 or above 64, NULL, a wrong kind on either table, tables on different devices, a broken
 * table, unknown flag bits.  Stream rule and transactionality: those of hbu_fold_harmonic. */
int hbu_fold_harmonic_lanes(hbu_table *lanes, hbu_table *centralities, double norm, uint32_t n_lanes, uint32_t flags, uint64_t *folded, uint64_t *inserted);

/* ---- the resident worker: its graph and its changed-node filter next to the tables ------------------------------------------------
 * In the reference a worker walks ALL of its edges every round and keeps those whose source passes its changed-nodes filter
 * (CentralityMapper::map_cardinalities, harmonic_centrality/mapper.rs:253-296, with a U64BloomFilter; ShortestPathMapper::relax_all_edges /
 * relax_exact_edges, shortest_path/mapper.rs:105-190, with an UpdatedNodes), then turns the returned actions into the next round's filter
 * (update_changed_nodes, mapper.rs:114-125; map_batch, shortest_path/mapper.rs:88-103).  With the calls below the graph and the filter
 * live on the device of the tables and one call per mapper step works between them: a round moves a few counts over the link, no ids.
 * Errors of the graph and filter calls are read with hbu_last_error(NULL) (the calling thread's last message); the round steps report
 * on the table that changes, as the edge steps do. */
typedef struct hbu_graph hbu_graph;
typedef struct hbu_filter hbu_filter;

#define HBU_FILTER_BLOOM 0 /* U64BloomFilter, crates/bloom/src/lib.rs:60-130                                       */
#define HBU_FILTER_EXACT 1 /* InnerUpdatedNodes::Exact, shortest_path/updated_nodes.rs:27-44: a set of whole 128-bit ids */

/* What worker.graph() yields (worker.rs:77-79), resident on one device: the nodes in host_nodes() order, the edges (from[i], to[i]) in the
 * worker's iteration order, edges with SKIPPED_REL flags already dropped by the caller (rel flags stay the worker's business).  Uploaded
 * once: 16 B per node, 32 B per edge.  Either list may be empty.  chunk_edges: the most edges (or nodes) one internal pass of a round
 * call handles, 0 = the library's default, >= 2^30 is HB_ERR_LIMIT.  The staging of a chunk (about 50 B per edge) is allocated by the
 * first round call that needs it, not here: a chunk the device has no room for is that call's HB_ERR_NOMEM, with nothing changed.  Chunking is invisible in tables and filters: the upserts apply
 * pairs in order, so consecutive chunks equal one batch for the counters, and a minimum is associative for the distances.  A graph keeps
 * the staging of one chunk: it serves one round call at a time. */
int hbu_graph_create(int32_t device, const hb_u128 *nodes, uint64_t n_nodes, const hb_u128 *from, const hb_u128 *to, uint64_t n_edges, uint64_t chunk_edges,
                     hbu_graph **out);
int hbu_graph_len(const hbu_graph *g, uint64_t *n_nodes, uint64_t *n_edges);
void hbu_graph_destroy(hbu_graph *g);

#define HBU_NODE_SKETCH_REGISTERS 4096
/* ShortestPathWorker::new (shortest_path/worker.rs:44-49): HyperLogLog<4096>::default() + add_u128(node) for every node of g;
 * registers_out: 4096 bytes.  add() is hyperloglog.rs:4385-4396 with b = 12: h = low 64 bits of the id * 11400714819323198549 mod 2^64
 * (the high half is ignored, hyperloglog.rs:4398-4400), register h >> 52 = max(itself, leading_zeros(h << 12) + 1), which is 65 where
 * h << 12 is zero.  An empty node list: 4096 zeros.  Registers only: merge() is a byte-wise max and size() stays with the caller. */
int hbu_graph_node_sketch(const hbu_graph *g, uint8_t *registers_out);

/* num_bits() of the bloom crate (lib.rs:40-42): ceil(items * ln(fp) / (-8 * ln(2)^2)) in that operation order, `as u64`.  Host only. */
uint64_t hbu_bloom_num_bits(uint64_t estimated_items, double fp);

/* HBU_FILTER_BLOOM: num_bits bits, 1 .. 2^32 - 1 (0: HB_ERR_INVALID, more: HB_ERR_LIMIT; a table holds fewer than 2^32 keys); the bit of
 * an id is (low 64 bits of the id * 11400714819323198549 mod 2^64) % num_bits, the high half is ignored as in insert_u128 /
 * contains_u128 (lib.rs:95-106).  HBU_FILTER_EXACT: num_bits is ignored. */
int hbu_filter_create(int32_t device, uint32_t kind, uint64_t num_bits, hbu_filter **out);
void hbu_filter_destroy(hbu_filter *f);
int hbu_filter_clear(hbu_filter *f);  /* empty_from (lib.rs:73-77, updated_nodes.rs:152-157) */
int hbu_filter_fill(hbu_filter *f);   /* fill() (lib.rs:79-83); bloom only */
int hbu_filter_insert(hbu_filter *f, const hb_u128 *ids, uint64_t count);
int hbu_filter_contains(hbu_filter *f, const hb_u128 *ids, uint64_t count, uint8_t *out_bytes);
/* dst |= src.  The kinds must match and, for blooms, num_bits too (the reference debug-asserts it, lib.rs:126): else HB_ERR_INVALID.
 * The Exact -> Sketch policy of UpdatedNodes::union / add (updated_nodes.rs:46-106) stays with the caller. */
int hbu_filter_union(hbu_filter *dst, hbu_filter *src);
int hbu_filter_count(hbu_filter *f, uint64_t *n); /* count_ones() of a bloom, len() of an exact set */
/* bloom only: the bit vector's data words, bit i = bit i % 64 of little-endian 64-bit word i / 64, ceil(num_bits / 64) words.  An import
 * whose tail bits above num_bits are not zero is refused.  The serde envelope stays with the caller. */
int hbu_filter_export_bits(hbu_filter *f, uint64_t *words_out);
int hbu_filter_import_bits(hbu_filter *f, const uint64_t *words);
/* exact only: the members, order unspecified; *written of them (HB_ERR_INVALID and nothing written if capacity is too small) */
int hbu_filter_export_ids(hbu_filter *f, hb_u128 *out, uint64_t capacity, uint64_t *written);

/* ---- the round steps.  All objects on one device; a call runs on next's stream and everything is visible on return.  Each call walks
 * the graph's lists in stored order, in chunks of at most chunk_edges.  Refused, nothing changed, hbu_last_error set on the table that
 * changes: NULL where an object is required, wrong table kinds, objects on different devices, prev == next, changed == new_changed, a
 * broken table.  An empty graph or a filter that selects nothing: HB_OK, zero counts, nothing touched.  A HIP error in the middle of a
 * multi-chunk call leaves each table as the batch calls leave it (the keys it held before the failing chunk, earlier chunks applied); the
 * error is reported and the caller redoes the round from its clone and a cleared new_changed. */

/* map_setup_counters (mapper.rs:211-242): prev and next both get batch_set(node, HyperLogLog::default() + add_u128(node)) for every
 * node of g, the counter derived on the device; every node is inserted into `changed` if that is not NULL. */
int hbu_setup_counters(hbu_table *prev_counters, hbu_table *next_counters, const hbu_graph *g, hbu_filter *changed);
/* map_cardinalities (mapper.rs:253-296): the edges whose from[e] `changed` contains, in stored order, applied exactly as
 * hbu_update_counters(prev, next, ...) applies them as one batch; the `to` of every pair whose action is Merged is inserted into
 * new_changed (mapper.rs:120-124: an Inserted destination is NOT).  *selected / *merged / *inserted: the selected edges and the pairs with
 * those actions; round_had_changes is merged + inserted > 0 (mapper.rs:141-147).  new_changed may be NULL, else it differs from changed. */
int hbu_round_counters(hbu_table *prev_counters, hbu_table *next_counters, const hbu_graph *g, hbu_filter *changed, hbu_filter *new_changed, uint64_t *selected,
                       uint64_t *merged, uint64_t *inserted);
/* RelaxEdges for the edges of g (shortest_path/mapper.rs:105-190): the same selection; each chunk's selected edges are applied as
 * hbu_update_distances applies them; every destination whose action is_changed() (Merged OR Inserted, upsert.rs:31-33, mapper.rs:97-101)
 * is inserted into new_changed.  *changed_nodes: the (destination, chunk) answers that were changed, > 0 iff the round had changes.  With
 * an HBU_FILTER_EXACT `changed` this selects exactly the edges relax_exact_edges reaches through
 * ForwardlinksQuery ... skip_self_links(false).deduplicate(false). */
int hbu_round_distances(hbu_table *prev_distances, hbu_table *next_distances, const hbu_graph *g, hbu_filter *changed, hbu_filter *new_changed, uint64_t *selected,
                        uint64_t *changed_nodes);
/* RelaxEdges (shortest_path/mapper.rs:105-190) for 64 sources in one pass over the edges of g; both tables HBU_KIND_DIST64.  Edge e is
 * selected iff `changed` contains from[e] AND from[e] has a row in prev (an edge whose source has none is skipped and inserts nothing, as in
 * hbu_update_distances).  Its pair is (to[e], cand) with cand[l] = prev[from[e]][l] + 1 on every lane that is not HBU_DIST_NONE and
 * HBU_DIST_NONE elsewhere; 254 + 1 is HBU_DIST_NONE, no candidate.  The row is gathered when the pair is folded; per edge only the source's
 * slot is staged.  The pairs are upserted into `next` with HBU_OP_DIST64_MIN in edge order (a candidate row of 64 x HBU_DIST_NONE like any
 * other: NoChange on a present key, Inserted on an absent one); to[e] of every pair whose action is_changed() (Merged OR Inserted) goes into
 * new_changed if that is not NULL.  *selected: the selected edges = the pairs; *merged / *inserted: the pairs with those actions; the round
 * had changes iff merged + inserted > 0.  Tables, counts and new_changed equal, bit for bit, those of hbu_batch_get_values(prev, from) of
 * the selected edges, the `+ 1` on the host and hbu_batch_upsert_values(next, HBU_OP_DIST64_MIN, to, ...).
 * Refusals: those of hbu_round_distances (NULL, a wrong kind on either table, different devices, prev == next, changed == new_changed, a
 * broken table: HB_ERR_INVALID, nothing changed, hbu_last_error on next).  Transactionality: that of hbu_round_distances (a HIP error in a
 * multi-chunk call leaves earlier chunks applied and next with the keys it held before the failing chunk).  Stream: the call runs on next's
 * stream after a synchronise of prev's and of both filters'; everything is visible on return.  Chunking is invisible: the pairs apply in
 * order and a minimum is associative. */
int hbu_round_lane_distances(hbu_table *prev, hbu_table *next, const hbu_graph *g, hbu_filter *changed, hbu_filter *new_changed, uint64_t *selected,
                             uint64_t *merged, uint64_t *inserted);
/* map_centralities (mapper.rs:298-333): the nodes of g that `changed` contains go through hbu_update_centralities, a chunk at a time;
 * *written sums the chunks' distinct nodes (the reference's batches are as separate). */
int hbu_round_centralities(hbu_table *prev_counters, hbu_table *next_counters, hbu_table *prev_centrality, hbu_table *next_centrality, const hbu_graph *g,
                           hbu_filter *changed, uint64_t round, uint64_t *selected, uint64_t *written);

/* ---- the finish of a job: what the two coordinators do with the finished centrality table (harmonic_centrality/coordinator.rs:204-233,
 * approximated_harmonic_centrality/coordinator.rs:152-177): the stored value, store_harmonic (webgraph/centrality/mod.rs:72-114) and
 * top_nodes (mod.rs:33-52).  `centrality` is HBU_KIND_KAHAN - the value is .sum = f64::from(KahanSum) (kahan_sum.rs:35-39), err is ignored -
 * or HBU_KIND_F64.  EVERY key of the table is a result whatever its value: negatives, -0.0, +inf (a sampled source's own distance folds as
 * inf) and NaNs are results like any other; hb_result_copy's "< 0 = absent" does not apply.  The result value is the IEEE quotient
 * value / divisor; no divisor is refused: the harmonic job passes (double)(num_nodes - 1), which is 0 for a one-key job, the approximated
 * job 1.0 (x / 1.0 is x).  The rank order is store_harmonic's (Reverse(SortableFloat(c)), NodeID): the quotient descending under
 * f64::total_cmp (+NaN > +inf > ... > +0.0 > -0.0 > ... > -inf > -NaN), ties by NodeID ascending (128-bit, unsigned) - hb_result_ranks'
 * definition.  The sign and payload of a NaN that the division creates are the device's (x86 and gfx950 produce different default NaNs),
 * and the ranks follow the values the call returns.
 * The table is only read and holds the same keys and values afterwards; everything is visible on return.  Refused with HB_ERR_INVALID and
 * hbu_last_error set (hbu_last_error(NULL) for a NULL table): a NULL table, a table of any other kind, a broken table, an empty `output`.
 * There is no result handle: each call derives what it needs by itself on the device (the keys by entry number, one 128-bit sort of the ids
 * carrying the entry number, the quotients and their sort keys in that order, one stable 64-bit sort), so three calls mean three times
 * those sorts. */

/* Entry j of the ascending-NodeID order (hb_result_copy's order, so the three arrays line up): ids_out[j], vals_out[j] = the quotient,
 * ranks_out[j] = its position in the rank order.  Any of the three may be NULL (all three: only *written is set).  *written = len (may be
 * NULL).  capacity < len with an output that is not NULL: HB_ERR_INVALID, nothing written.  An empty table: HB_OK, *written = 0. */
int hbu_finish_centralities(hbu_table *centrality, double divisor, hb_u128 *ids_out, double *vals_out, uint64_t *ranks_out, uint64_t capacity,
                            uint64_t *written);
/* top_nodes as hb_result_top defines it: the first min(k, len) entries of the rank order, gathered on the device - only they cross the link.
 * ids_out / vals_out: room for min(k, len) entries, either may be NULL.  *written = min(k, len).  k = 0: HB_OK, *written = 0. */
int hbu_top_centralities(hbu_table *centrality, double divisor, uint64_t k, hb_u128 *ids_out, double *vals_out, uint64_t *written);
/* store_harmonic: the databases `harmonic` (NodeID -> f64) and `harmonic_rank` (NodeID -> u64) under `output`, byte for byte what
 * hb_store_harmonic(output, ids, vals, ranks, len, ...) writes from the arrays of hbu_finish_centralities; the key order of the databases
 * (ascending bincode key bytes) comes from the device as in hb_store_harmonic_results, from the ids the device already holds: values, ranks
 * and the sorted key records come down, no id does.  Failures are the writer's own (HB_ERR_IO ...): nothing is left behind, no meta.json
 * appears before both databases are complete, and the call can be repeated.  err (may be NULL): the message, as hbu_last_error has it. */
int hbu_store_centralities(hbu_table *centrality, double divisor, const char *output, char *err, uint64_t err_len);

#ifdef __cplusplus
}
#endif
#endif /* HB_AMPC_H */
