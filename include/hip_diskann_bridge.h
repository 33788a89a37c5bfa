/*
 * hip_diskann_bridge.h — C ABI for DiskANN batch distances on MI355X.
 *
 * Signature-identical replacement of the reference's Metal bridge
 * (src/include/metal_diskann_bridge.h:8-23, implemented in src/metal_diskann_bridge.mm:155-323,
 * stubbed in src/metal_diskann_stub.cpp:9-24).  Callers in the reference:
 *   - rust_lib/src/metal_ffi.rs:10-30 (→ DiskProvider::search / search_batch,
 *     rust_lib/src/disk_provider.rs:417-445, :590-627; Provider::search_batch, provider.rs:385-415)
 *   - src/ann_search.cpp:723-732 (vector_distances → ComputeDistances)
 *
 * Semantics (diskann_distance.metal:15-194, rust_lib/src/distance.rs:15-24):
 *   metric 0 = L2  → out[i] = Σ_j (q_j − c_j)²           (squared Euclidean)
 *   metric 1 = IP  → out[i] = −Σ_j q_j · c_j             (negated dot; lower = more similar)
 * Returns 0 on success, −1 on invalid arguments (n/total_n/nq/dim ≤ 0, NULL pointers, a metric
 * other than 0/1, a query_map entry ≥ nq) or device failure; the caller then computes on the CPU
 * (disk_provider.rs:436-453, provider.rs:407-426).  Calls are synchronous; the caller owns all
 * buffers and nothing is retained after return.  Unlike the Metal bridge (non-atomic ring index,
 * metal_diskann_bridge.mm:52-53, :119-120) every entry point is thread-safe: each calling thread
 * gets its own stream and staging buffers.
 *
 * For drop-in linking the library also exports the reference's own `diskann_metal_*` names
 * (aliases of the `diskann_hip_*` functions), so rust_lib's metal_ffi.rs links unchanged.
 *
 * Extension: an HBM-resident database and an id-based call, so a
 * lock-step BFS step ships only candidate ids (4 B) instead of candidate vectors (4·dim B).
 * fmt 0 = fp32 rows (n*dim floats); fmt 1 = SQ8 codes (n*dim uint8) with per-dimension `sq8_min`
 * and `sq8_scale` (dequant v = (q/255)·scale + min, rust_lib/src/provider.rs:140-146, :161-210).
 */
#ifndef HIP_DISKANN_BRIDGE_H
#define HIP_DISKANN_BRIDGE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Returns 1 if HIP DiskANN acceleration is available, 0 otherwise (metal_diskann_bridge.h:8). */
int diskann_hip_available(void);

/* One query (dim floats) vs n contiguous candidates (n*dim floats) → out_distances[n]
 * (metal_diskann_bridge.h:10-15). */
int diskann_hip_batch_distances(const float *query, const float *candidates, int n, int dim, int metric,
                                float *out_distances);

/* nq queries (nq*dim), total_n candidates (total_n*dim); candidate i is compared with
 * queries[query_map[i]] (metal_diskann_bridge.h:17-23). */
int diskann_hip_multi_batch_distances(const float *queries, const float *candidates, const unsigned int *query_map,
                                      int total_n, int nq, int dim, int metric, float *out_distances);

/* Drop-in aliases of the reference names (same semantics as the diskann_hip_* functions). */
int diskann_metal_available(void);
int diskann_metal_batch_distances(const float *query, const float *candidates, int n, int dim, int metric,
                                  float *out_distances);
int diskann_metal_multi_batch_distances(const float *queries, const float *candidates, const unsigned int *query_map,
                                        int total_n, int nq, int dim, int metric, float *out_distances);

/* ---- extension: HBM-resident database + id gather ---------------------------------------- */

#define DISKANN_HIP_FMT_F32 0
#define DISKANN_HIP_FMT_SQ8 1

/* Upload n vectors (fmt as above) to HBM on the current device; returns a handle or NULL. */
void *diskann_hip_register_db(const void *data, int64_t n, int dim, int fmt, const float *sq8_min,
                              const float *sq8_scale);

/* out[i] = dist(queries[query_map[i]], db[ids[i]]) for i < total_n.  ids ≥ n are an error (−1).
 * Host pointers; synchronous. */
int diskann_hip_multi_batch_distances_ids(void *db, const float *queries, int nq, const unsigned int *ids,
                                          const unsigned int *query_map, int total_n, int metric,
                                          float *out_distances);

/* Same with every buffer already in HBM (asynchronous on `stream`, a hipStream_t; NULL = the
 * default/null stream).  For benchmarking the kernel with resident inputs. */
int diskann_hip_multi_batch_distances_ids_device(void *db, const float *queries_dev, int nq,
                                                 const unsigned int *ids_dev, const unsigned int *query_map_dev,
                                                 int total_n, int metric, float *out_dev, void *stream);

/* Lock-step multi-query best-first search over the registered DB — DiskProvider::search_batch
 * (rust_lib/src/disk_provider.rs:470-652: pop the best candidate per active query, stop when
 * |result| >= L and it is worse than result[L-1], expand unvisited neighbours, insert_result
 * :656-678) with every step's distances computed by the id-gather kernel.  adjacency: n*R uint32,
 * padded with UINT32_MAX (rust_lib/src/file_format.rs:3-18).  Outputs nq*k labels (−1 past the
 * result) and distances (FLT_MAX past the result).  stats (may be NULL): [0] distance evaluations,
 * [1] lock-step iterations, [2] GPU calls, [3] reserved.  Returns 0 / −1 (message in err_buf). */
int diskann_hip_search_batch(void *db, const uint32_t *adjacency, int R, const uint32_t *entry_points, int n_ep,
                             const float *queries, int nq, int k, int l_search, int metric, int64_t *out_ids,
                             float *out_dists, int64_t *stats, char *err_buf, int err_len);

/* ---- extension: GPU-resident traversal ---------------------------------------------------------
 * The whole DiskProvider::search_batch (disk_provider.rs:470-678) on the device: one wavefront per
 * query runs the reference's state machine (sorted result list of L, pop of the smallest unexpanded
 * (dist, id), neighbour expansion up to the first u32::MAX, visited set, insert_result with Rust's
 * binary_search_by) against the HBM-resident DB and adjacency — no per-step host round trip.
 * Results equal diskann_hip_search_batch's up to fp32 summation order.  Shapes the kernel does not
 * cover (R > 64, n_ep > 64, L > 256, d beyond 2048 SQ8 / 2048 fp32 or not a multiple of 16 / 4) and
 * the rare query whose boundary-tie spill list overflows run through the host BFS transparently.
 * stats (may be NULL): [0] distance evaluations, [1] max BFS steps over queries (the lock-step count),
 * [2] node expansions (pops) on the GPU, [3] queries re-run on the host. */

/* Upload the graph (n x R uint32 adjacency, padded with UINT32_MAX) next to the registered DB. */
int diskann_hip_register_graph(void *db, const uint32_t *adjacency, int R);

/* Host pointers; synchronous. */
int diskann_hip_search_batch_resident(void *db, const uint32_t *entry_points, int n_ep, const float *queries, int nq,
                                      int k, int l_search, int metric, int64_t *out_ids, float *out_dists,
                                      int64_t *stats, char *err_buf, int err_len);

/* queries / out_ids / out_dists in HBM; launched on `stream` (hipStream_t, NULL = the DB's stream); returns
 * after the traversal finished (it reads back the per-query flags). */
int diskann_hip_search_batch_resident_device(void *db, const uint32_t *entry_points, int n_ep,
                                             const float *queries_dev, int nq, int k, int l_search, int metric,
                                             int64_t *out_ids_dev, float *out_dists_dev, int64_t *stats, void *stream,
                                             char *err_buf, int err_len);

/* ---- extension: graph build on the device -------------------------------------------
 * Batched insert + RobustPrune + back-edge update against the registered fp32 DB, in the handle's graph metric
 * (below).  Refused with a message (never a slow path): a `metric` other than the handle's graph metric, an SQ8 DB,
 * R > 64, L > 256, L < 1, d % 4 != 0, d > 2048, n >= 2^31, alpha < 1 or NaN, entry_point >= n, batch_max < 1.  A
 * refused call leaves a registered graph as it was. */

/* The metric of the graph a handle builds and maintains: 0 (L2, the default) or 1 (IP; the prune is the crate's
 * occluding rule).  An index has one metric for life, so it is a property of the handle:
 * diskann_hip_build_graph, _robust_prune, _add_rows and _remove_ids require their `metric` argument to equal it (on a
 * handle never told otherwise that is L2, and metric = 1 is refused as before), diskann_hip_batch_mates uses it, and
 * diskann_hip_quantize_sq8 copies it onto the new handle.  It may be set at any time, before or after a graph is
 * registered; it is taken under the handle's mutex and changes nothing in HBM.  The search entry points keep their
 * per-call `metric` and do not read it.  set: 0, or -1 (NULL, or a value other than 0 / 1; message in err_buf).
 * get: the metric, or -1 for NULL. */
int diskann_hip_set_graph_metric(void *db, int metric, char *err_buf, int err_len);
int diskann_hip_graph_metric(void *db);

/* Build the graph of the registered fp32 DB on the device (spec: DESIGN §6).  adjacency_out: n*R uint32 (host, may be NULL).
 * On success the graph is also registered on `db`, as after diskann_hip_register_graph.  stats (may be NULL, 8 int64):
 * [0] search distance evaluations, [1] batches, [2] out-edge prunes, [3] back-edge prunes, [4] searches re-run on the
 * host, [5] pools truncated to 256, [6] rows unreachable from entry_point, [7] reserved.  0 / -1 (message in err_buf). */
int diskann_hip_build_graph(void *db, int R, int l_build, float alpha, int metric, uint32_t entry_point,
                            int batch_max, uint32_t *adjacency_out, int64_t *stats, char *err_buf, int err_len);

/* prune() of the spec (prune_ip() of DESIGN §6.5 on an IP handle) for m targets: pools is m*pool_cap ids (UINT32_MAX-padded; self, repeats and ids >= n are
 * dropped), distances to the target computed on the device.  out: m*R ids, UINT32_MAX-padded.  Host pointers; synchronous. */
int diskann_hip_robust_prune(void *db, const uint32_t *targets, int m, const uint32_t *pools, int pool_cap, int R,
                             float alpha, int metric, uint32_t *out, char *err_buf, int err_len);

/* Measurement: host seconds of the last diskann_hip_build_graph on `db`, per phase: [0] searches, [1] out-edge
 * prunes, [2] back-edges (grouping, appends, prunes).  seconds: 3 doubles. */
int diskann_hip_build_phase_seconds(void *db, double *seconds);

/* ---- extension: row removal from the device graph ---------------------------------
 * FreshDiskANN's delete consolidation on the registered fp32 DB and graph, in place of a rebuild of the survivors
 * (InMemoryIndex::compact, rust_lib/src/index_manager.rs:687-716).  labels: host int64, any order; duplicates and
 * labels outside [0, n) are ignored.  Only the live rows that point at a removed row are repaired: their pool is
 * their live neighbours plus the live neighbours of their removed neighbours (one hop), pruned as in the build.
 * Then the rows and the adjacency are compacted: survivors keep their order, new id = old id − removed rows below
 * it (the label_map `compact` returns), every stored id is relabelled.  A removed entry point is replaced by the
 * nearest live row, (Σ(a−b)², id) ascending — (−dot, id) on a handle whose graph metric is IP.
 * Refused with a message (never a slow path): whatever the build refuses (a `metric` other than the handle's graph
 * metric, an SQ8 DB, R > 64, d % 4 != 0,
 * d > 2048, n >= 2^31, alpha < 1 or NaN), no graph registered, *entry_point >= n, removing every row.  A refused or
 * failed call leaves the handle answering as before.  No label in range: returns 0 and nothing moves.
 * scratch_words: pool slots (uint32) the repair may hold at once, 0 = 2^28; the result does not depend on it.
 * adjacency_out: room for n*R (the old n); the first n'*R words are written.  stats (may be NULL, 8 int64): [0] rows
 * removed, [1] rows repaired (pruned), [2] pools truncated to 256, [3] live ids gathered into pools, [4] slabs,
 * [5] 1 when the entry point was replaced, [6] rows the new entry point does not reach, [7] reserved.
 * Synchronous, on the DB's stream under the DB's mutex.  Returns the rows removed, or -1 (message in err_buf).
 * Against registering the survivors and a full diskann_hip_build_graph the call was the faster one at every removed
 * fraction measured (1, 10 and 30 % of 100K x 128 at R 64, L 128 on one MI355X, equal recall@10:
 * profiles/diskann_remove/README.md), so no fraction is known above which a rebuild is the better call.  Beyond 30 %
 * removed, and at other shapes, nothing is measured. */
int64_t diskann_hip_remove_ids(void *db, const int64_t *labels, int64_t n_labels, float alpha, int metric,
                               uint32_t *entry_point /* in: old id, out: new id */,
                               int64_t scratch_words /* 0 = default */,
                               uint32_t *adjacency_out /* n' * R, host, may be NULL */,
                               int64_t *stats /* 8, may be NULL */, char *err_buf, int err_len);

/* Measurement: seconds of the last diskann_hip_remove_ids on `db`: [0] pool build (host time of mark, rank, pool
 * lengths and the slab plan, plus the pool fills' device time), [1] the prunes' device time, [2] the rest of the
 * call (entry point, compaction, copies to the host).  seconds: 3 doubles. */
int diskann_hip_remove_phase_seconds(void *db, double *seconds);

/* ---- extension: row insertion into the device graph ---------------------------------
 * Appends m fp32 rows (host, m*dim) to the registered DB and inserts them into its registered graph — the device
 * counterpart of InMemoryIndex::add (rust_lib/src/index_manager.rs:262-313), in place of register_db + build_graph
 * over all rows.  The rows get ids n .. n+m-1 in order (the labels `next_label` assigns).  Batches follow the build's
 * rule continued, b = min(batch_max, rows in the graph, rows left); each batch is searched against the graph as it
 * stood at the batch's start, pruned and back-linked as in the build.  batch_mates = T > 0 adds every batch row's
 * min(T, b-1) nearest other batch rows to its prune pool, so that a burst of mutually similar rows links to itself
 * (without it such rows only see the old graph); T = 0 is bit for bit the build's own loop continued.
 * Refused with a message (never a slow path): whatever the build refuses (a `metric` other than the handle's graph
 * metric, an SQ8 DB, d % 4 != 0, d > 2048, alpha < 1 or NaN), no graph registered, L outside [1, 256], batch_max < 1, batch_mates outside [0, 64],
 * L + batch_mates > 512, entry_point >= n, rows NULL with m > 0, n + m >= 2^31, a non-finite value in rows.  A refused
 * call leaves the handle answering as before; m = 0 returns 0 and nothing moves.  A device failure after the first
 * change cannot be rolled back: the handle keeps its n rows but drops its graph, and searches refuse until a graph is
 * registered or built again.
 * Device storage grows by a quarter when it is full (rows, adjacency, repeated-id bits), so repeated small calls are
 * amortised.  The host copy of the adjacency is not refreshed unless adjacency_out is given ((n+m)*R words, host):
 * a one-row call copies nothing of the graph back.  stats (may be NULL, 8 int64): [0] search distance evaluations,
 * [1] batches, [2] out-edge prunes, [3] back-edge prunes, [4] searches re-run on the host, [5] pools truncated to 256,
 * [6] rows unreachable from entry_point (-1 when adjacency_out is NULL: the walk needs the host copy), [7] mate ids
 * written.  Synchronous, on the DB's stream under the DB's mutex.  Returns the new n, or -1 (message in err_buf).
 * Measured against register_db + build_graph over all rows (100K x 128, R 64, L 128, batch_max 4096, 16 mates, one
 * MI355X, both in one process, adjacency read back; profiles/diskann_add/README.md): 0.09 / 0.21 / 0.46 of the
 * rebuild's time at 1 / 10 / 30 % added on i.i.d. rows, 0.09 / 0.19 / 0.45 for added rows from new cluster centres,
 * where recall@10 on queries like the added rows is 1.00 / 1.00 / 0.999 with mates, 0.53 / 0.86 / 0.95 without and
 * 0.54 / 0.95 / 0.96 for the rebuild.  The mates step is 1 - 5 % of the call (0.45 ms per batch of 4096 against 1.2 ms
 * of out-edge prunes).  One row into the 100K-row graph: 2.2 ms without adjacency_out, 15 - 21 ms with it.  Other
 * shapes, and fractions above 30 %, are not measured. */
int64_t diskann_hip_add_rows(void *db, const float *rows, int64_t m, int l_build, float alpha, int metric,
                             uint32_t entry_point, int batch_max, int batch_mates,
                             uint32_t *adjacency_out /* (n+m) * R, host, may be NULL */,
                             int64_t *stats /* 8, may be NULL */, char *err_buf, int err_len);

/* The mates step of add_rows alone, over the registered rows row0 .. row0+b-1 (fp32 DB, d % 4 == 0, d <= 2048,
 * 1 <= T <= 64): out[i*T + j] = the id of the j-th nearest other row of the range to row row0+i, ordered by
 * (max(0, (G_ii + G_jj) - 2 G_ij), id) with G the range's Gram matrix — by (-G_ij, id) on a handle whose graph metric
 * is IP —; UINT32_MAX past min(T, b-1).  Host pointer; synchronous. */
int diskann_hip_batch_mates(void *db, int64_t row0, int b, int T, uint32_t *out /* b * T */, char *err_buf,
                            int err_len);

/* Measurement: host seconds of the last diskann_hip_add_rows on `db`, per phase: [0] searches, [1] mates,
 * [2] out-edge prunes, [3] back-edges.  seconds: 4 doubles. */
int diskann_hip_add_phase_seconds(void *db, double *seconds);

/* ---- extension: entry point and SQ8 search copy computed on the device -----------------
 * One or two streaming passes over the rows the handle already holds, so the lifecycle needs the rows on the device
 * once: register -> medoid -> build_graph -> quantize_sq8 -> SQ8 resident search -> add_rows / remove_ids -> quantize
 * again (the codec's min / max are global, so a re-quantize is the whole pass).  Both device calls take the source's
 * mutex, run on its stream and read its n rows only; neither changes the source.  No floating-point atomics and a row
 * split that depends on n alone: two runs give the same bits. */

/* Row nearest the mean of the registered fp32 rows (L2; smallest id on a tie) — hipann.medoid on the device:
 * c = (sum of the rows) / n and the distances sum_j (double(x_ij) - c_j)^2 in fp64, the smallest (distance, id).  Every
 * dim >= 1.  Refused: NULL, an SQ8 handle, n = 0.  0 / -1 (message in err_buf). */
int diskann_hip_medoid(void *db, uint32_t *row_out, char *err_buf, int err_len);

/* Provider::quantize_sq8 (provider.rs:161-210) on the device: a NEW handle, fmt SQ8, holding the codes of the
 * source's n fp32 rows, min/scale per dimension, and — when the source has a graph registered — a device-to-device
 * copy of its adjacency (same R), ready for every call an SQ8 handle takes today.  The source is not changed.
 * Codec, in fp32: min[j], max[j] over the n rows; scale[j] = max - min if that is > 0, else 1;
 * code = (u8) clamp(roundf(((v - min[j]) / scale[j]) * 255.0f), 0, 255) (IEEE division, round half away from zero).
 * The handle is filled as diskann_hip_register_db(fmt = SQ8) fills it; the host copy of the adjacency is read back only
 * when a flagged query needs the host BFS.  A source without a graph gives a handle without one.
 * Refused with a message (never a slow path): a NULL or SQ8 source, n = 0, a non-finite value in the rows.
 * Returns the handle (release with diskann_hip_release_db) or NULL (message in err_buf). */
void *diskann_hip_quantize_sq8(void *db, char *err_buf, int err_len);

/* Codes (n*dim u8), min[dim], scale[dim] of an SQ8 handle back to the host, for the SQ8\0 trailer
 * (index_manager.rs:513-533).  Any output may be NULL.  Refused: a NULL or fp32 handle.  0 / -1. */
int diskann_hip_export_sq8(void *db, void *codes /* n*dim uint8 */, float *sq8_min, float *sq8_scale, char *err_buf,
                           int err_len);

/* Measurement: seconds of the last diskann_hip_quantize_sq8 from `db`: [0] column statistics, [1] encode,
 * [2] the rest (finite check, graph copy, handle set-up).  3 doubles. */
int diskann_hip_quantize_phase_seconds(void *db, double *seconds);

int64_t diskann_hip_db_size(void *db);

/* Measurement: record HIP events around every id-gather kernel launch of `db` (on its stream) from now
 * on (on != 0; resets the record), and read back the summed kernel time and the launch count. */
int diskann_hip_set_kernel_timing(void *db, int on);
int diskann_hip_kernel_stats(void *db, double *total_ms, int64_t *launches);
void diskann_hip_release_db(void *db);

#ifdef __cplusplus
}
#endif

#endif /* HIP_DISKANN_BRIDGE_H */
