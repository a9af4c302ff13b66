/*
 * hvs.h -- C ABI of the MI355X-native filtered brute-force k-NN engine (libhvs.so).
 *
 * Drop-in boundary for ONE path of atalantus/Project---Hybrid-Vector-Search-Queries:
 * the `vec_query` seam every engine header of the reference defines
 *     void vec_query(vector<vector<float>>& nodes, vector<vector<float>>& queries,
 *                    float sample_proportion, vector<vector<uint32_t>>& knn_results);
 * (reference include/optimized_parallel.hpp:61-62, include/optimized.hpp:54-55,
 * include/baseline.hpp:68-69; called once from src/test.cpp:85) together with the
 * binary formats of include/io.h (D rows = 102 f32 [C,T,x0..x99], Q rows = 104 f32
 * [type,v,l,r,x0..x99], output.bin = nq x 100 uint32 ids in ascending distance).
 *
 * std::vector cannot cross a C ABI, so the boundary takes flat row-major buffers; the
 * header-only shim include/hvs_vec_query.hpp restores the exact C++ signature.
 *
 * Conventions: plain pointers and sizes, no exceptions, int status (0 = ok, negative =
 * HVS_E*), one hvs_ctx is used from one thread at a time (the reference has a single
 * caller, src/test.cpp:85).  A context is one GPU (hvs_create) or all GPUs of the node
 * (hvs_create_multi); per GPU the engine runs on the context's own HIP stream, hvs_query's
 * host transfers on two more (copy-in, copy-out), and a multi-GPU context drives each GPU
 * from its own host thread for the duration of a call.  dim = 100 is a compile-time constant like the reference's VEC_DIM (include/optimized_impl.h:28);
 * k defaults to the reference's KNN_LIMIT = 100 (optimized_impl.h:26) and can be changed per context (hvs_set_k).
 */
#ifndef HVS_H
#define HVS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HVS_OK 0
#define HVS_EINVAL (-1)  /* bad argument (NULL, n < 100, nq range ...) */
#define HVS_ENOMEM (-2)  /* host or device allocation failed */
#define HVS_EHIP (-3)    /* a HIP runtime call failed; see hvs_last_error */
#define HVS_ESTATE (-4)  /* call order: no data / no queries / no results loaded */

typedef struct hvs_ctx hvs_ctx;

/* Engines.  HVS_ENGINE_AUTO picks the fastest exact engine for the loaded data. */
#define HVS_ENGINE_AUTO 0
#define HVS_ENGINE_EXACT_SCAN 1 /* FP32 exact-order scan of every candidate row (VALU)       */
#define HVS_ENGINE_MFMA_FILTER 2 /* BF16 MFMA bound filter + exact-order re-scoring (same answers) */
#define HVS_ENGINE_MFMA_I8 3     /* INT8 MFMA bound filter + exact-order re-scoring (same answers); falls back to
                                    a 16-bit float filter for data the INT8 format cannot bound */
#define HVS_ENGINE_MFMA_F16 4    /* FP16 MFMA bound filter + exact-order re-scoring (same answers): the BF16 filter's cost,
                                    an 8x tighter bound; what HVS_ENGINE_AUTO picks for clustered / low-dimensional data */

typedef struct hvs_timing {
    double query_ms;      /* whole vec_query-equivalent region on the device stream (HIP events)   */
    double main_kernel_ms;/* sum of the dominant kernel's launches inside that region               */
    uint32_t main_kernel_launches;
    uint32_t nq;          /* queries answered                                                       */
    uint64_t pairs;       /* sum over queries of rows in [0,sn) passing the predicate (P of SURVEY 8d) */
    uint64_t scanned_pairs;/* (query,row) pairs the dominant kernel actually evaluated              */
    double load_ms;       /* last hvs_load_data / hvs_gen_data: upload + index build                */
    uint32_t engine;      /* engine that ran                                                        */
    uint32_t fallback_queries; /* queries re-run by the exact scan after a filter overflow          */
    uint64_t rescored_pairs;   /* MFMA engine: (query,row) pairs handed to the exact re-scoring kernel */
    uint32_t n_gpus;      /* GPUs that took part (multi-GPU context: query_ms = the slowest GPU's, counters summed)   */
    uint32_t untimed_launches; /* launches of the dominant kernel that could not be timed (event creation failed):
                                  main_kernel_ms is then a lower bound and must not feed a roofline                    */
    double host_ms;       /* last hvs_query: wall time of the whole call, host memory in -> host memory out (the
                             reference's timing scope, src/test.cpp:82-88); 0 for the device-resident calls          */
    uint32_t retry_queries;    /* filter engines: queries whose guessed threshold failed its check and that were run
                                  again with a proven one (same answers either way)                                     */
    uint32_t flags;            /* HVS_TIMING_* bits                                                                     */
} hvs_timing;
#define HVS_TIMING_INDEX_TOO_LARGE 1u /* the data set has more than 2^29 rows per GPU: no filter index, exact engine only */
#define HVS_TIMING_I8_ROTATED 4u      /* the INT8 tiles that ran were cut from the rotated vectors (csrc/hvs_filter.h, HvsQuant): same answers */
#define HVS_TIMING_FORMAT_CHANGED 2u  /* HVS_ENGINE_AUTO: so many queries of this call had no usable INT8 bound (far outside the
                                         data's box) that the 16-bit float tiles were built in mid-call; later calls use them */

/* ---- lifetime ---------------------------------------------------------------------------- */

/* One GPU.  device < 0: use the calling thread's current HIP device. */
int hvs_create(hvs_ctx **out, int device);
/* All GPUs of the node behind ONE context -- what the reference's vec_query does with the cores of the machine
 * (optimized_parallel.hpp:73-89: it sizes and owns its worker pool itself).  n_gpus = 0: every visible GPU.  D is
 * replicated (one upload over PCIe, GPU-to-GPU copies over xGMI), the queries of a call are cut into one contiguous
 * range per GPU (optimized_parallel.hpp:91: iterations are independent), one host thread drives each GPU, and every GPU
 * writes its block of ids straight into its slice of the caller's out_ids -- no collective.  Every function below
 * accepts such a context unless it says "single-GPU contexts only". */
int hvs_create_multi(hvs_ctx **out, int n_gpus);
/* The same on an explicit device list; an index may repeat ("virtual ranks": several parts on one GPU -- how the
 * multi-GPU plan is tested on a one-GPU box). */
int hvs_create_on_devices(hvs_ctx **out, const int *devices, int n);
int hvs_num_gpus(const hvs_ctx *ctx);
/* GPUs visible to this process (0 when there is none: the library has no CPU fallback). */
int hvs_device_count(void);
/* How hvs_query of a multi-GPU context brings the ids home.  DIRECT (default): each GPU's pipeline D2H-copies into its
 * slice of the caller's array.  PEER: the blocks travel GPU -> GPU 0 over xGMI and leave in one D2H (A/B partner; a
 * process-per-GPU driver gathers with RCCL instead, bench.py / sharding.py). */
#define HVS_GATHER_DIRECT 0
#define HVS_GATHER_PEER 1
int hvs_set_gather(hvs_ctx *ctx, int mode);
/* Announce the size of the coming calls: query/result buffers and the per-batch workspace (~34 GB for batches of 2^21
 * queries) are allocated now (and again after a later hvs_load_data) instead of inside the first query. */
int hvs_reserve(hvs_ctx *ctx, uint32_t nq);
void hvs_destroy(hvs_ctx *ctx);
/* Message of the last failing call on this context ("" if none). Valid until the next call. */
const char *hvs_last_error(const hvs_ctx *ctx);
/* Library-level message for failures that have no context (hvs_create). */
const char *hvs_last_global_error(void);
int hvs_set_engine(hvs_ctx *ctx, int engine);
/* Summation order of the distances.  HVS_ORDER_SIMD (default) is the hot path's AVX2 order
 * (optimized_impl.h:96-125) used by optimized.hpp / optimized_parallel.hpp; HVS_ORDER_SCALAR is the
 * sequential order of the reference's baseline engine (baseline.hpp:53-64; BASELINE.json configs[0]),
 * answered by the exact engine.  The two orders give different f32 distances and, now and then,
 * different neighbours (reference optimized.hpp:34-42). */
#define HVS_ORDER_SIMD 0
#define HVS_ORDER_SCALAR 1
int hvs_set_distance_order(hvs_ctx *ctx, int order);
/* Neighbours per query: the reference's compile-time KNN_LIMIT (include/optimized_impl.h:26, static_assert >= 8),
 * a run-time property here.  8 <= k <= 256, default 100; every "100" in the layouts below reads "k" after the call
 * (out_ids / out_dists rows hold k entries, the data set needs n >= k rows, padding appends rows n-1, n-2, ... up to
 * k).  Results of earlier queries are dropped. */
int hvs_set_k(hvs_ctx *ctx, uint32_t k);
uint32_t hvs_get_k(const hvs_ctx *ctx);
/* Padding (default on) appends rows n-1, n-2, ... when fewer than 100 rows match
 * (optimized_parallel.hpp:149-157).  A context that holds only a SHARD of D (D-sharded multi-GPU mode,
 * sharding.py) turns it off: unmatched slots then carry id 0xFFFFFFFF / distance +inf and the merge of
 * the shards' partial answers applies the padding once, from the tail of the whole data set. */
int hvs_set_padding(hvs_ctx *ctx, int enabled);

/* ---- data set D (replaces `nodes`, reference src/test.cpp:71-73 + io.h:111-136) ---------- */

/* rows: host memory, n x 102 f32.  Requires n >= 100 (the reference's padding index n-s
 * underflows below that, optimized.hpp:125).  Uploads and builds the device-side layout. */
int hvs_load_data(hvs_ctx *ctx, const float *rows, uint32_t n);
/* Generate gen-v1 rows (include/hvs_gen.h) directly in HBM. */
int hvs_gen_data(hvs_ctx *ctx, uint32_t n, uint64_t seed, int profile, uint32_t ncat);
/* Copy raw rows [row0,row0+nrows) back to the host (n x 102 layout). */
int hvs_download_data(hvs_ctx *ctx, uint32_t row0, uint32_t nrows, float *out_rows);
uint32_t hvs_num_rows(const hvs_ctx *ctx);

/* ---- the vec_query seam ------------------------------------------------------------------ */

/*
 * q_rows: host, nq x 104 f32.  out_ids: host, nq x 100 u32 (output.bin row layout, ascending
 * distance, canonical tie rule (dist asc, id asc)).  out_dists: host, nq x 100 f32 exact-order
 * distances of those ids, or NULL.  sample_proportion as in the reference: rows [0, sn) are
 * searched with sn = uint32(float(sample_proportion) * float(n)) (optimized_parallel.hpp:67);
 * padding ids come from the end of the full set (n-1, n-2, ...), optimized_parallel.hpp:149-157.
 * The call is a pipeline: queries go to the GPU in pieces through pinned staging slots one batch ahead of the engine,
 * finished batches' ids come back while the next batch computes (buffers the caller pinned itself skip the staging
 * copies).  hvs_last_timing().host_ms is the wall time of the whole call.
 */
int hvs_query(hvs_ctx *ctx, const float *q_rows, uint32_t nq, float sample_proportion, uint32_t *out_ids,
              float *out_dists);

/* ---- device-resident variant (benchmarks, multi-GPU drivers: inputs already in HBM) ------ */

int hvs_upload_queries(hvs_ctx *ctx, const float *q_rows, uint32_t nq);
int hvs_gen_queries(hvs_ctx *ctx, uint32_t nq, uint64_t seed, int profile, uint32_t ncat, int force_type,
                    uint64_t first_row);
int hvs_download_queries(hvs_ctx *ctx, uint32_t q0, uint32_t nq, float *out_rows);
/* Answer resident queries [q0, q0+nq); results stay on the device (rows q0..q0+nq of the result
 * buffer).  Asynchronous on the context stream(s); hvs_sync waits (and lets the exact engine re-run the few queries
 * whose filter lists overflowed, if any). */
int hvs_query_resident(hvs_ctx *ctx, uint32_t q0, uint32_t nq, float sample_proportion);
int hvs_sync(hvs_ctx *ctx);
int hvs_download_results(hvs_ctx *ctx, uint32_t q0, uint32_t nq, uint32_t *out_ids, float *out_dists);
/* Copy result rows [q0,q0+nq) into caller-owned DEVICE buffers (same GPU), e.g. a collective's
 * send buffer.  d_dists may be NULL.  Asynchronous on the context stream.  Single-GPU contexts only. */
int hvs_export_results_device(hvs_ctx *ctx, uint32_t q0, uint32_t nq, uint32_t *d_ids, float *d_dists);
/* Stream-ordered hand-off: work enqueued on `stream` (a hipStream_t of the context's GPU, e.g. the stream a collective
 * runs on) after this call starts only when everything the context has enqueued so far is complete -- no host wait for
 * the kernels (queries the filter left unanswered are re-run first, which costs the call's one host synchronisation).
 * Single-GPU contexts only. */
int hvs_stream_wait(hvs_ctx *ctx, void *stream);
/* D-sharded mode (rows partitioned over GPUs, every GPU answers all queries on its rows with hvs_set_padding(ctx, 0)):
 * merges the shards' partial answers on the device -- the multi-GPU counterpart of Knn::merge (reference
 * include/optimized_impl.h:337-385) -- and applies the reference's padding (optimized_parallel.hpp:149-157) once.
 * d_ids_all / d_dists_all: DEVICE, [nshards][nq][100] as an all_gather of the per-shard results lays them out (ids
 * shard-local, 0xFFFFFFFF = empty slot); shard_row0: HOST, first global row of each shard (nshards <= 16);
 * d_pad_dists: DEVICE, [nq][100], exact-order distance of query q to row n_total-1-s; outputs: DEVICE, [nq][100], global
 * ids in ascending (dist, id) order (d_out_dists may be NULL).  Asynchronous on the context stream.  Single-GPU
 * contexts only. */
int hvs_merge_shards_device(hvs_ctx *ctx, uint32_t nshards, uint32_t nq, const uint32_t *d_ids_all,
                            const float *d_dists_all, const uint64_t *shard_row0, uint32_t n_total,
                            const float *d_pad_dists, uint32_t *d_out_ids, float *d_out_dists);
/* Timing of the last hvs_query / hvs_query_resident (call after hvs_sync).  HVS_ESTATE when there is none to report: before
 * the first call, after hvs_set_k and hvs_compact, and after any index build in which the planner of HVS_ENGINE_AUTO ran its
 * probe batch (a load, hvs_reindex or a fold of 32768 rows and more): the probe uses the call's counters, and the per-call
 * figures of hvs_mask_stats / hvs_append_stats / hvs_update_stats read zero until the next call. */
int hvs_last_timing(hvs_ctx *ctx, hvs_timing *out);
/* Diagnostics: which queries of the last call were answered a second time (call after hvs_sync / hvs_query).
 * which = 0: the exact engine's list (hvs_timing.fallback_queries), 1: the retry list (hvs_timing.retry_queries).
 * Copies up to cap query indices (relative to the call's resident query set) to out_idx and returns the list's length,
 * or a negative HVS_E* code.  Single-GPU contexts only. */
int hvs_last_reruns(hvs_ctx *ctx, int which, uint32_t *out_idx, uint32_t cap);

/* Host-side planning rules, exposed for tests (pure arithmetic: no GPU, no context).
 * hvs_plan_guess_m: the order statistic m of a guessed threshold (csrc/hvs_filter.h, "Guessed thresholds") for k neighbours when
 * a fraction `seen_fraction` of the query's rows has been seen and one guess may fail with probability 10^-pfail.
 * hvs_plan_batches: the batch sizes hvs_query (host_pipeline != 0) or hvs_query_resident cuts a call of nq queries into for
 * the filter engines; writes up to cap sizes to out (may be NULL) and returns their number. */
uint32_t hvs_plan_guess_m(uint32_t k, double seen_fraction, uint32_t pfail);
uint32_t hvs_plan_batches(uint32_t nq, int host_pipeline, uint32_t *out, uint32_t cap);

const char *hvs_version(void);

/* ---- row deletion: a live-row mask (tombstones) ------------------------------------------ */

/*
 * "Deleted" means "as if the row had never been in D, with ids unchanged".  Let `live` be the ascending list of ids
 * that are not deleted, n_live its length and D' the rows D[live] in that order: for every engine, distance order, k,
 * padding mode and sample_proportion the answer of a call on (D, mask) is the answer of the same call on D' with every
 * id j replaced by live[j].  So the rows searched are the first uint32(float(sample_proportion) * float(n_live)) live
 * rows, padding appends live[n_live-1], live[n_live-2], ..., a deleted id appears in no output slot, and
 * hvs_timing.pairs counts live rows only.  n_live >= k is required as n >= k is: a mask change (or hvs_set_k) that would
 * break it returns HVS_EINVAL and leaves the context as it was.  hvs_load_data / hvs_gen_data reset the mask to "all
 * live".  While no row is dead every call runs exactly the kernels it runs without these functions.
 * All of them accept a multi-GPU context (the mask is replicated to every GPU, like D).  The D-sharded mode
 * (sharding.py, hvs_merge_shards_device) knows nothing of masks: a shard context may carry a mask of its own, but the
 * merge pads from the tail of the whole data set as before.
 */
typedef struct hvs_mask_info {
    uint32_t n_live;         /* rows that are not deleted                                                            */
    uint32_t n_dead;         /* rows that are                                                                        */
    uint64_t tiles_patched;  /* rows whose filter-tile entry carries the format's never-hit encoding, summed over both
                                orderings (2 n_dead once the tiles of a filter engine are built and patched)          */
    uint64_t dead_survivors; /* last call: filter survivors the re-scoring front end dropped because the row is dead  */
} hvs_mask_info;
/* ids: host memory.  Duplicates and ids that are dead already are fine; an id >= n is HVS_EINVAL and nothing is applied. */
int hvs_delete_rows(hvs_ctx *ctx, const uint32_t *ids, uint32_t count);
/* live_bits: host memory, ceil(n / 64) words, bit (i & 63) of word (i >> 6) set = row i is live.  Replaces the whole
 * mask (rows may come back).  NULL: all rows live. */
int hvs_set_row_mask(hvs_ctx *ctx, const uint64_t *live_bits);
int hvs_get_row_mask(hvs_ctx *ctx, uint64_t *live_bits);
uint32_t hvs_num_live_rows(const hvs_ctx *ctx);
/* Call after hvs_sync / hvs_query.  Multi-GPU context: the mask's and tiles' figures of one GPU (they are replicated),
 * dead_survivors summed over the GPUs. */
int hvs_mask_stats(hvs_ctx *ctx, hvs_mask_info *out);
/* The host arithmetic of the contract (no GPU, no context; live_bits NULL = all live; any output may be NULL):
 * n_live = popcount; cut = live[sn_live] with sn_live = uint32(float(sample_proportion) * float(n_live)), or n when
 * sn_live == n_live -- the rows searched are "id < cut and live"; pad_ids[0..k) = the last k live ids in descending
 * order (0xFFFFFFFF where n_live < k). */
void hvs_mask_plan(const uint64_t *live_bits, uint32_t n, uint32_t k, float sample_proportion, uint32_t *n_live,
                   uint32_t *cut, uint32_t *pad_ids);

/* ---- row append: new rows searchable at once, the index folded in later ---------------------- */

/*
 * After hvs_append_rows(ctx, rows, count, &first_id) the context behaves, in every later call on every engine, as a fresh
 * context would after hvs_load_data of the old rows followed by the new ones under the same settings (engine, k, distance
 * order, padding, and the mask extended with live rows): the same ids -- appended rows get n_old .. n_old + count - 1 --,
 * bit-equal out_dists, the same (dist asc, id asc) tie rule, the same hvs_timing.pairs.  So
 * sn = uint32(float(sample_proportion) * float(n_total)) is taken over the total, padding comes from n_total - 1,
 * n_total - 2, ... (from the last live ids under a mask), hvs_num_rows / hvs_download_data see the new rows, appended rows
 * start live, hvs_delete_rows / hvs_set_row_mask accept their ids and hvs_get_row_mask returns ceil(n_total / 64) words.
 * The index (orderings, filter tiles) keeps covering the rows it was built over, ids [0, n_indexed); the rows behind it, the
 * tail, are scanned in exact order for every batch that goes through the index.  An append that would leave more than
 * tail_limit rows in the tail re-indexes over all rows before it returns; hvs_reindex does so on request; no query ever does.
 * While the tail is empty -- or lies wholly behind sn -- every call runs exactly the kernels it runs without these
 * functions.  Without an index (fewer than 4096 rows, or no room for one) appends only extend D, n_tail stays 0, and an
 * index is built by the same limit rule once the data set allows one.
 * count == 0: HVS_OK, nothing changes.  rows == NULL or more than 2^32 - 1 rows: HVS_EINVAL; no data loaded: HVS_ESTATE; no
 * room: HVS_ENOMEM; in each of these cases the context, D, the mask and the index are as they were.  (Any other failure --
 * a HIP error while the rows are copied or the index is rebuilt -- is reported as it is and may leave the context without an
 * index, or the GPUs of a multi-GPU context with different row counts: load the data again.)  hvs_load_data /
 * hvs_gen_data reset everything (tail empty, counters 0) but the limit.  All of these functions accept a multi-GPU context:
 * rows and state are replicated like D and the mask, and room is secured on every GPU before any GPU changes.  The
 * D-sharded mode (sharding.py, hvs_merge_shards_device) knows nothing of appends, as it knows nothing of masks.
 */
typedef struct hvs_append_info {
    uint32_t n_indexed;     /* rows the orderings/tiles cover (0: no index, the exact engine scans everything) */
    uint32_t n_tail;        /* rows behind them: n_total - n_indexed when an index exists, else 0              */
    uint32_t tail_limit;    /* n_tail above which hvs_append_rows re-indexes before it returns                  */
    uint32_t reindexes;     /* index builds caused by appends or hvs_reindex since the last load                */
    uint64_t tail_pairs;    /* last call: (query, tail row) pairs the tail scan evaluated (re-run batches apart) */
    uint64_t tail_admitted; /* last call: of those, keys that entered a candidate list                         */
    double   reindex_ms;    /* last such build                                                                  */
} hvs_append_info;
int hvs_append_rows(hvs_ctx *ctx, const float *rows /* host, count x 102 */, uint32_t count, uint32_t *first_id /* may be NULL */);
/* room for D (and the mask) to grow to n_capacity rows without a device-to-device move */
int hvs_reserve_rows(hvs_ctx *ctx, uint32_t n_capacity);
/* fold the tail into the index now (no-op when n_tail == 0) */
int hvs_reindex(hvs_ctx *ctx);
/* rows; 0: the default rule max(4096, n_indexed / 1024) */
int hvs_set_tail_limit(hvs_ctx *ctx, uint32_t rows);
/* Call after hvs_sync / hvs_query.  Multi-GPU context: one GPU's state (it is replicated), the two per-call counters summed. */
int hvs_append_stats(hvs_ctx *ctx, hvs_append_info *out);
/* The host arithmetic of the contract (no GPU, no context; any output may be NULL): for an index over n_indexed of n_total
 * rows and a sample_proportion, sn and the id range [tail_lo, tail_hi) = [n_indexed, max(n_indexed, sn)) the tail scan covers
 * (empty when sn <= n_indexed). */
void hvs_append_plan(uint32_t n_indexed, uint32_t n_total, float sample_proportion, uint32_t *sn, uint32_t *tail_lo,
                     uint32_t *tail_hi);

/* ---- row update in place: ids kept, new contents searchable at once -------------------------- */

/*
 * After hvs_update_rows(ctx, ids, rows, count) the context behaves, in every later call on every engine, as a fresh context
 * would after hvs_load_data of the current rows with row ids[i] replaced by rows[i], under the same settings (engine, k,
 * distance order, padding, mask): the same ids, bit-equal out_dists, the same (dist asc, id asc) tie rule, the same
 * hvs_timing.pairs.  All 102 floats of a row change, C and T included: an updated row may enter or leave any query's
 * predicate.  Liveness does not change: a dead row stays dead with its new contents, and a later hvs_set_row_mask that
 * revives it shows the new contents.  n, sn, the cut and the padding ids are untouched; hvs_download_data returns the new
 * contents.  Duplicates in ids are applied in order: the last one wins.
 * A row with id in [n_indexed, n) (the tail), or any row of a context without an index, is only overwritten in D.  An indexed
 * row (id < n_indexed) that is updated becomes STALE: the orderings and tiles still describe its old contents, so the index
 * treats it as dead (its tile entries are tombstoned like a deleted row's) and every batch that goes through the index scans
 * the stale rows below sn by id, in exact order, next to the tail.  Queries never re-index.  The limit is shared with the
 * tail: an update -- or an append -- that would leave n_tail + n_stale > tail_limit re-indexes over all rows before it
 * returns; hvs_reindex does so on request (also when only stale rows are left to fold in); either clears the stale set and
 * counts in hvs_append_info.reindexes.  hvs_load_data / hvs_gen_data reset the stale set.  While no indexed row is stale every
 * call runs exactly the kernels it runs without this function.
 * count == 0: HVS_OK, nothing changes.  ids == NULL, rows == NULL or any ids[i] >= n: HVS_EINVAL; no data loaded: HVS_ESTATE;
 * no room: HVS_ENOMEM; in each of these cases the context, D, the mask and the index are as they were.  Any other failure is
 * reported as hvs_append_rows reports it.  The call accepts a multi-GPU context: rows and state are replicated like D and the
 * mask, and room is secured on every GPU before any GPU changes.  The D-sharded mode (sharding.py, hvs_merge_shards_device)
 * knows nothing of updates, as it knows nothing of masks or appends.
 * While rows are stale hvs_mask_info.tiles_patched counts their tile entries too, and dead_survivors keeps counting dead rows
 * only: a survivor dropped because its row is stale (and live) is counted in stale_survivors.
 */
typedef struct hvs_update_info {
    uint32_t n_stale;          /* indexed rows whose index entry describes old contents                              */
    uint32_t limit;            /* n_tail + n_stale above which an update or append re-indexes (= tail_limit)         */
    uint64_t stale_pairs;      /* last call: (query, stale row) pairs the stale scan evaluated (re-run batches apart) */
    uint64_t stale_admitted;   /* last call: of those, keys that entered a candidate list                             */
    uint64_t stale_survivors;  /* last call: filter survivors dropped because the row's index entry is stale          */
} hvs_update_info;             /* 32 bytes */
int hvs_update_rows(hvs_ctx *ctx, const uint32_t *ids, const float *rows /* host, count x 102 */, uint32_t count);
/* Call after hvs_sync / hvs_query.  Multi-GPU context: one GPU's state (it is replicated), the three per-call counters summed. */
int hvs_update_stats(hvs_ctx *ctx, hvs_update_info *out);
/* host arithmetic, no GPU, no context: fold one call's ids into the ascending stale list.  Returns the new length, or
 * 0xFFFFFFFF (nothing written) if any id >= n_total.  out_stale (room for n_stale + count): ascending, unique, ids >=
 * n_indexed left out.  out_last[i] (count entries, may be NULL) = 1 where occurrence i is the last of its id. */
uint32_t hvs_update_plan(const uint32_t *stale, uint32_t n_stale, const uint32_t *ids, uint32_t count,
                         uint32_t n_indexed, uint32_t n_total, uint32_t *out_stale, uint8_t *out_last);

/* ---- row compaction: dead rows dropped from D, live rows renumbered, one index over them ------ */

/*
 * Let `live` be the ascending list of live ids and n_live its length.  After hvs_compact(ctx, map) returns HVS_OK the context
 * behaves, in every later call on every engine, as a fresh context would after hvs_load_data of the current rows D[live] in
 * that order under the same settings (engine, k, distance order, padding, tail limit) -- "current" meaning the contents
 * hvs_update_rows left, appended rows included.  So row live[j] now has id j, out_dists are bit-equal to the fresh load's
 * under the same (dist asc, id asc) tie rule, hvs_timing.pairs is the same, hvs_num_rows is n_live, sn and the padding ids
 * are taken over the new n; the mask is "all live" (n_dead = 0: every call runs the unmasked kernels again, hvs_get_row_mask
 * returns ceil(n_live / 64) words of ones); the stale set and the tail are empty under one index over all rows; and
 * hvs_delete_rows, hvs_update_rows, hvs_append_rows (first new id = n_live) and hvs_download_data speak the new ids at once.
 * map[j] = live[j] is written before anything on the device changes.  Results of earlier queries hold old ids and are
 * dropped as hvs_set_k drops them; resident queries stay.  An earlier call's pending re-runs are resolved first, under the
 * old mask.  The index build counts in hvs_append_info.reindexes / reindex_ms; hvs_timing.load_ms stays the load's.
 * No dead row: HVS_OK and nothing changes -- tail and stale rows stay, no re-index, the map is the identity, `compactions`
 * is not incremented.  Nothing compacts on its own: ids belong to the caller.
 * The rows move in place (row live[j] to place j <= live[j], rows below the first dead id untouched) through a bounce buffer
 * of one chunk of HVS_COMPACT_CHUNK source rows (default 65536), so the call needs no second copy of D.  The capacity of D
 * (hvs_reserve_rows) is kept: the next appends need no growth.  hvs_trim_rows gives it back: D is re-allocated to exactly n
 * rows (no-op when it has no spare room; needs n rows of spare room while it runs; HVS_ENOMEM: the context is as it was).
 * No data loaded: HVS_ESTATE; no room for the scratch buffers: HVS_ENOMEM; in both cases the context, D, the mask and the
 * index are as they were.  Any other failure is reported as hvs_append_rows reports it: load the data again.  Multi-GPU
 * contexts are accepted: every GPU compacts its replica, and room is secured on every GPU before any GPU changes.  The
 * D-sharded mode knows nothing of compaction.
 */
typedef struct hvs_compact_info {
    uint32_t compactions;   /* since the last load                                            */
    uint32_t n_before, n_after; /* last compaction                                            */
    uint32_t first_moved;   /* last: smallest old id whose row changed place (= first dead id) */
    uint32_t chunks;        /* last: gather launches                                          */
    uint64_t rows_moved;    /* last: live rows with old id > first_moved                      */
    double   move_ms;       /* last: device time of the row move (HIP events), index build apart */
} hvs_compact_info;
int  hvs_compact(hvs_ctx *ctx, uint32_t *new_to_old /* host, n_live entries, may be NULL */);
/* Multi-GPU context: one GPU's figures. */
int  hvs_compact_stats(hvs_ctx *ctx, hvs_compact_info *out);
int  hvs_trim_rows(hvs_ctx *ctx);
/* The host arithmetic (no GPU, no context; live_bits NULL = all live; any output may be NULL): n_live = popcount,
 * first_dead = the first clear bit (n when there is none), new_to_old = the ascending live ids. */
void hvs_compact_plan(const uint64_t *live_bits, uint32_t n, uint32_t *n_live, uint32_t *first_dead,
                      uint32_t *new_to_old /* n_live entries, may be NULL */);

/* ---- row-partitioned context: one D cut over the GPUs -------------------------------------------- */

/*
 * hvs_create_multi / hvs_create_on_devices keep all of D on every GPU and cut the queries.  A row-partitioned context cuts D:
 * part r (one GPU; a device index may repeat, "virtual ranks") holds the contiguous global rows [row0[r], row0[r+1]) =
 * shard_range(n, r, n_parts) and nothing else of D but a replica of its last min(n, 256) rows; every part holds all resident
 * queries and answers all of them on its rows.  The resident queries are cut into one owner range per part (the same
 * shard_range rule); after the parts have finished a call, each owner copies the other parts' partial lists of its queries
 * (device-to-device copies, no collective), merges them by the key order (dist asc, id asc) and applies the reference's
 * padding once.  So a data set may be n_parts times what one GPU holds, and the filter index covers 2^29 rows PER PART.
 *
 * The contract: after hvs_load_data / hvs_gen_data on a partitioned context, every later hvs_query, hvs_query_resident +
 * hvs_download_results returns what a one-GPU context (hvs_create) returns for the same rows under the same settings (engine,
 * k, distance order, padding): the same ids, bit-equal out_dists, the same hvs_timing.pairs.
 *  - Sampled prefix: sn = uint32(float(sample_proportion) * float(n)) is taken over the whole n; part r searches its first
 *    local_sn[r] rows (hvs_partition_plan); a part with local_sn == 0 launches nothing.  The rule "filter engines only while
 *    the prefix is at least a quarter of the rows" holds per part: every engine gives the same answers.
 *  - Padding comes from global rows n-1, n-2, ..., duplicates of matched rows included, exactly as on one GPU; with
 *    hvs_set_padding(ctx, 0) unmatched slots are 0xFFFFFFFF / +inf.
 *  - hvs_num_rows returns n, hvs_num_gpus n_parts, hvs_num_live_rows n; hvs_download_data serves ranges that cross parts;
 *    hvs_upload_queries / hvs_gen_queries / hvs_query put all queries on every part; hvs_reserve(nq) sizes every part for all
 *    nq queries plus the exchange buffers; hvs_query_resident blocks the host until the merged answers exist (the call's one
 *    synchronisation); hvs_last_timing reports the slowest part's query_ms plus exchange_ms plus merge_ms, nq of the call,
 *    counters summed over the parts, flags OR-ed.  Every part picks engine, index and tile format from ITS rows, so the parts of
 *    one call may run different engines: hvs_timing.engine is that of the last part (highest r) that searched rows in the call
 *    (HVS_ENGINE_EXACT_SCAN when none did), fallback_queries, retry_queries and rescored_pairs are the parts' sums -- none of
 *    these need equal a one-GPU context's figures; ids, out_dists and pairs do.
 *  - Every part must hold at least k rows: a load with n < n_parts * k, or an hvs_set_k that would break the rule, returns
 *    HVS_EINVAL and leaves the context as it was.
 *  - Not supported (yet) on a partitioned context, HVS_ESTATE and nothing changes: row deletion, append, update and compaction
 *    (hvs_delete_rows, hvs_set_row_mask, hvs_get_row_mask, hvs_append_rows, hvs_reserve_rows, hvs_reindex, hvs_set_tail_limit,
 *    hvs_update_rows, hvs_compact, hvs_trim_rows), their *_stats functions, hvs_set_queries_from_rows and hvs_set_gather.  The functions that say
 *    "single-GPU contexts only" refuse it as they refuse any multi-GPU context.
 *  - A call that fails half-way reports the failing part like any multi-GPU call and leaves no kernel running.
 */
int hvs_create_partitioned(hvs_ctx **out, const int *devices, int n_parts);   /* 1..16 parts; an index may repeat (virtual ranks) */
typedef struct hvs_partition_info {
    uint32_t n_parts;
    uint32_t row0[17];          /* part r holds global rows [row0[r], row0[r+1]) -- shard_range(n, r, n_parts) */
    uint32_t padded_queries;    /* last call: queries that matched fewer than k rows in all parts together      */
    uint64_t exchanged_bytes;   /* last call: bytes of partial lists copied between parts                       */
    double   exchange_ms, merge_ms; /* last call: slowest part's device time of the list copies / of the merge kernel */
} hvs_partition_info;
int hvs_partition_stats(hvs_ctx *ctx, hvs_partition_info *out);   /* HVS_ESTATE on a context that is not partitioned */
/* host arithmetic, no GPU, no context; any output may be NULL: row0[0..n_parts] = the parts' first rows, sn = uint32(float(sp) * float(n)),
   local_sn[r] = min(max(sn, row0[r]), row0[r+1]) - row0[r] = rows of part r inside the sampled prefix.  Returns 0, or HVS_EINVAL
   (n_parts outside 1..16, or a part with fewer than k rows). */
int hvs_partition_plan(uint32_t n, uint32_t n_parts, uint32_t k, float sample_proportion, uint32_t *row0, uint32_t *sn, uint32_t *local_sn);

/* ---- device-resident inputs: D and queries from GPU memory, queries from stored rows ------------- */

/*
 * The input side of the device-resident calls above (hvs_query_resident, hvs_export_results_device, hvs_stream_wait): rows that
 * already sit in HBM -- a model's embeddings, a collective's receive buffer, another kernel's output -- enter the context
 * without a round trip through host memory.  Every context kind accepts the two *_device calls.
 *
 * The buffer: plain device memory (hipMalloc and what is built on it) of ANY GPU visible to the process; the call finds the GPU
 * with hipPointerGetAttributes, and the pointer may lie anywhere inside an allocation.  Host memory of any kind -- pageable,
 * pinned, managed -- is HVS_EINVAL: nothing changes (resident queries, results and D are as they were) and the runtime's own
 * error is cleared, the next call does not trip over it.  `stream`: a hipStream_t of the buffer's GPU, NULL = its null stream;
 * the work enqueued on it so far is complete before the buffer is read.  The calls block: they return when the copies are done
 * (as hvs_upload_queries / hvs_load_data do), the buffer is only read and is the caller's again on return.
 *
 * hvs_set_queries_device(ctx, d_q_rows, nq, stream): afterwards the context is in every respect the context after
 * hvs_upload_queries of the same bytes -- the same hvs_download_queries, the same owner ranges on a multi-GPU context, the same
 * answers from hvs_query_resident.  One GPU: one device-to-device (or peer) copy; hvs_create_multi contexts: every GPU takes its
 * range of the queries straight from the buffer; row-partitioned contexts: every part takes all nq rows.  nq == 0: HVS_OK and an
 * empty resident set (the pointer is not looked at); d_q_rows == NULL with nq > 0: HVS_EINVAL.
 *
 * hvs_load_data_device(ctx, d_rows, n, stream): afterwards the context is the context after hvs_load_data of the same bytes --
 * the same checks before anything changes (n >= k; n >= n_parts * k on a partitioned context), the same resets (mask, tail,
 * stale set, counters, hvs_last_timing), the same index; hvs_timing.load_ms is the copy plus the index build.  Every GPU copies
 * from the buffer itself: all n rows, or, as part r of a partitioned context, its rows shard_range(n, r, n_parts) and its replica
 * of the last min(n, 256) rows.
 *
 * hvs_set_queries_from_rows(ctx, ids, first_id, nq, type, dt): "the neighbours of rows I already stored".  Resident query i is
 * built on the device from row ids[i] (ids == NULL: row first_id + i) as D holds it NOW -- the contents hvs_update_rows left,
 * appended rows included, the new ids after hvs_compact --: its 100 vector floats are the row's, bit for bit, and its
 * attributes follow the row's category C and timestamp T by `type`, each of l = T - dt and r = T + dt being one IEEE f32
 * operation (a NaN that comes out of it has an unspecified payload: such a query matches nothing either way).  The query set is
 * a snapshot: a later change of D does not touch it.  The answers are those of hvs_upload_queries of the rows hvs_row_query
 * builds from hvs_download_data.  Self-matches are not removed: the row is in D, so with HVS_ROWQ_KNN a live row with finite
 * components is its own nearest neighbour at distance 0, and the other types find it whenever it lies inside the sampled prefix.
 * ids: HOST memory, duplicates are fine.  HVS_EINVAL and nothing changes (resident queries and results are as they were): type
 * outside 0..3, dt negative or NaN, an id >= n, an id that is deleted under the live-row mask ("as if it had never been in D").
 * No data loaded: HVS_ESTATE.  nq == 0: HVS_OK and an empty resident set.  hvs_create_multi contexts: every GPU builds its range
 * of the queries from its own replica.  Row-partitioned contexts: HVS_ESTATE, not supported (yet) -- a query's source row lives
 * on one part and every part needs every query; that exchange is a later step.
 *
 * hvs_row_query: the host arithmetic of that rule for one row (no GPU, no context; type in 0..3) -- the same function the kernel
 * calls for the four attribute floats.
 */
int hvs_set_queries_device(hvs_ctx *ctx, const float *d_q_rows /* device, nq x 104 */, uint32_t nq, void *stream);
int hvs_load_data_device(hvs_ctx *ctx, const float *d_rows /* device, n x 102 */, uint32_t n, void *stream);
#define HVS_ROWQ_KNN      0   /* [0, -1, -1, -1]          */
#define HVS_ROWQ_SAME_C   1   /* [1,  C, -1, -1]          */
#define HVS_ROWQ_T_WINDOW 2   /* [2, -1, T - dt, T + dt]  */
#define HVS_ROWQ_BOTH     3   /* [3,  C, T - dt, T + dt]  */
int hvs_set_queries_from_rows(hvs_ctx *ctx, const uint32_t *ids /* host, nq entries, or NULL */, uint32_t first_id, uint32_t nq,
                              int type, float dt);
void hvs_row_query(const float *row /* 102 */, int type, float dt, float *out_q /* 104 */);

/* ---- per-query distance caps: the k nearest rows within a radius ---------------------------------- */

/*
 * "The k nearest rows that pass the predicate -- and are no farther than r": a cap is one f32 per resident query, max_d2[q], a
 * SQUARED L2 distance, compared with the engine's exact-order f32 distance as `dist <= max_d2[q]` in IEEE arithmetic.  The output
 * stays [nq][k]; the cap is a third predicate beside C and T.
 *  - A row takes part in query q's answer only if it passes the query's predicate, lies in the sampled prefix, is live and is
 *    within the cap.  Everything else is as if the rows beyond the cap did not match: the slots they leave are padded from n-1,
 *    n-2, ... (from the last live ids under a mask) -- pad rows need not be within the cap, as they need not pass the predicate --
 *    and with hvs_set_padding(ctx, 0) those slots are empty (0xFFFFFFFF / +inf).  The tie rule (dist asc, id asc), the ids and
 *    the distance bits are unchanged, and hvs_timing.pairs keeps counting predicate-passing rows: it does not look at the cap.
 *  - The matched rows of a query in key order have the rows within the cap as a prefix.  So the capped answer with padding off
 *    is the uncapped answer with padding off with every slot where !(dist <= cap) made empty; with padding on those slots are
 *    then filled by the padding rule (hvs_within_plan is that arithmetic).
 *  - A row whose distance is NaN is within no cap, +inf included.  A cap that is NaN or negative matches nothing.
 *  - "No cap" is expressed by not setting caps (or removing them), NOT by a cap of +inf: the two differ exactly for rows whose
 *    distance is NaN, which an uncapped query may return and a cap of +inf excludes.
 * While no caps are set every call runs exactly the kernels it runs without these functions.  The caps are a PROVEN threshold the
 * filter engines start from (instead of +inf): a tight radius prunes at every level.  Every engine, both distance orders, every
 * k, the live-row mask, appended and updated rows compose with caps; the D-sharded mode (sharding.py) knows nothing of them.
 *
 * hvs_set_max_dist2(ctx, max_d2, nq): attaches caps (HOST memory, nq floats) to the resident query set.  nq must equal the
 * number of resident queries: otherwise HVS_EINVAL and nothing changes (caps already set stay in force).  max_d2 == NULL removes
 * the caps (nq is not looked at).  Any call that replaces the resident set removes them too -- hvs_upload_queries,
 * hvs_gen_queries, hvs_set_queries_device, hvs_set_queries_from_rows and hvs_query -- so every call sequence without these
 * functions behaves as before.  Results of earlier calls stay in place.  Multi-GPU contexts cut the caps by the queries' owner
 * ranges; a row-partitioned context puts all caps on every part (the parts' lists then hold keys within the cap only and the
 * merge pads as it always does).
 * hvs_set_max_dist2_device: the same from DEVICE memory, by the rules of hvs_set_queries_device -- plain device memory of any
 * visible GPU, `stream` = the stream that produced it (NULL: the null stream), host memory of any kind is HVS_EINVAL with the
 * runtime's error cleared, the call blocks until the copy is done.
 * hvs_query_within: hvs_query with caps (host, nq floats: 4 bytes per query, sent whole before the pipeline starts); the caps
 * stay attached to the call's queries afterwards.  max_d2 == NULL behaves exactly as hvs_query.
 * hvs_within_stats: figures of the last call (after hvs_sync / hvs_query); HVS_ESTATE where hvs_last_timing has none to report.
 * Multi-GPU contexts: summed.  Row-partitioned contexts: capped_queries is the call's, underfull_queries the merge's count of
 * queries with fewer than k keys in all parts together, and within_slots the sum of the PARTS' non-pad slots -- every part
 * answers every query on its rows, so a query whose parts hold more than k rows within the cap between them counts more than k.
 */
typedef struct hvs_within_info {
    uint32_t capped_queries;    /* queries of the last call that carried a cap (all of them, or none)  */
    uint32_t underfull_queries; /* of those, queries with fewer than k rows within their cap           */
    uint64_t within_slots;      /* non-pad slots over all capped queries                               */
} hvs_within_info;
int hvs_set_max_dist2(hvs_ctx *ctx, const float *max_d2 /* host, nq */, uint32_t nq);
int hvs_set_max_dist2_device(hvs_ctx *ctx, const float *d_max_d2 /* device, nq */, uint32_t nq, void *stream);
int hvs_query_within(hvs_ctx *ctx, const float *q_rows, const float *max_d2, uint32_t nq, float sample_proportion, uint32_t *out_ids,
                     float *out_dists);
int hvs_within_stats(hvs_ctx *ctx, hvs_within_info *out);
/* The host arithmetic of the contract for one answer row (no GPU, no context; any output may be NULL).  ids / dists: k slots of
 * an UNCAPPED, UNPADDED answer (empty slots 0xFFFFFFFF / +inf); pad_ids / pad_dists: the first k padding rows (ids n-1, n-2, ...
 * or the last live ids, and their exact-order distances; unused, may be NULL, when `padding` is 0).  out_ids / out_dists: the
 * capped row -- the slots within the cap, then padding or empty slots, in (dist asc, id asc) order; n_within: slots within. */
void hvs_within_plan(const uint32_t *ids, const float *dists, uint32_t k, float max_d2, const uint32_t *pad_ids, const float *pad_dists,
                     int padding, uint32_t *out_ids, float *out_dists, uint32_t *n_within);

/* ---- per-query result cursors: the k nearest rows after a given key -------------------------------- */

/*
 * "The k nearest rows that pass the predicate -- and come AFTER this key": a cursor is one key per resident query, the pair
 * (after_dist f32, after_id u32), compared in the engines' own key order: distance bits ascending, then id ascending; +inf
 * after every finite value, the canonical NaN (0x7FC00000) after +inf.  It is the lower bound that the distance cap is the
 * upper bound of, and with it top-K for any K is a loop of pages of k, each of them exact.
 *  - A row takes part in query q's answer only if it passes the query's predicate, lies in the sampled prefix, is live, is
 *    within the cap if caps are set, and its key (dist, id) is STRICTLY greater than the cursor's.  Everything else is as if
 *    the rows at or before the cursor did not match: the slots they leave are padded from n-1, n-2, ... (from the last live ids
 *    under a mask) or are empty (0xFFFFFFFF / +inf) with hvs_set_padding(ctx, 0).  hvs_timing.pairs keeps counting
 *    predicate-passing rows: it does not look at cursors.  Ids, distance bits and the tie rule are unchanged.
 *  - The paging law.  Let full(q) be all matched keys of query q in key order.  The answer with cursor c and padding off is the
 *    first k keys of full(q) that are > c, then empty slots.  So page p+1, run with the cursor set to the last slot of page p,
 *    continues full(q) exactly where page p stopped: the concatenation of pages 1..P is the first P*k keys of full(q), with no
 *    gap and no repeat -- rows with equal distances and duplicate rows included, the id decides.
 *  - A cursor with after_id == 0xFFFFFFFF means "exhausted" and matches nothing, whatever its distance: that is what the last
 *    slot of an under-full, unpadded page holds, so feeding each row's last slot back is always right with padding off, and an
 *    exhausted query stays exhausted.  A NaN after_dist is taken as the canonical NaN key.
 *  - "No cursor" is expressed by not setting cursors (or removing them), never by a special value.  While no cursors are set
 *    every call runs exactly the kernels it runs without these functions.
 *  - The cursor is a key, not a row reference: the row it names may have been deleted or updated since.
 * Cursors compose with caps, the live-row mask, appended and updated rows, every engine, both distance orders and every k; the
 * D-sharded mode (sharding.py) knows nothing of them.  They belong to the resident query set exactly as caps do: any call that
 * replaces the set -- hvs_upload_queries, hvs_gen_queries, hvs_set_queries_device, hvs_set_queries_from_rows, hvs_query --
 * removes them.  Results of earlier calls stay in place.  A cursor gives the filter engines nothing to prune with (it bounds
 * the distance from below); it is tested wherever a key enters a candidate list.
 *
 * hvs_set_after(ctx, after_dists, after_ids, nq): attaches cursors (HOST memory, nq entries each).  nq must equal the number
 * of resident queries: otherwise HVS_EINVAL and nothing changes.  Both pointers NULL removes the cursors (nq is not looked
 * at); exactly one NULL is HVS_EINVAL.  Multi-GPU contexts cut the cursors by the queries' owner ranges; a row-partitioned
 * context puts all of them on every part (after_id is a GLOBAL row id; each part translates it to its own rows).
 * hvs_set_after_device: the same from DEVICE memory, by the rules of hvs_set_max_dist2_device -- plain device memory of any
 * visible GPU (both buffers on the same one), `stream` = the stream that produced them (NULL: the null stream), host memory of
 * any kind is HVS_EINVAL with the runtime's error cleared, the call blocks until the copies are done.
 * hvs_set_after_from_results: every resident query's cursor becomes slot k-1 of its current result row, on the device, with
 * no host round trip.  Requires that results for ALL resident queries exist (with the current k) and that padding is off --
 * with padding on the last slot may be a pad row --, otherwise HVS_ESTATE and nothing changes.  Replicated multi-GPU context:
 * each GPU does its own range.  Row-partitioned context: each owner's last slots travel to every part by device-to-device
 * copies on the parts' streams (8 bytes per query).
 * hvs_query_after: hvs_query with cursors, and optionally caps (max_d2 may be NULL), sent whole before the pipeline starts;
 * they stay attached to the call's queries afterwards.  Both after_* NULL behaves as hvs_query_within; exactly one NULL is
 * HVS_EINVAL.
 * hvs_after_stats: figures of the last call (after hvs_sync / hvs_query); HVS_ESTATE where hvs_last_timing has none to report.
 * Summed over a multi-GPU context; on a row-partitioned one by the rules of hvs_within_stats (cursor_queries the call's,
 * underfull_queries the merge's, after_slots the sum of the parts' non-pad slots), exhausted_queries counted once.
 */
typedef struct hvs_after_info {
    uint32_t cursor_queries;    /* queries of the last call that carried a cursor (all of them, or none) */
    uint32_t exhausted_queries; /* of those, queries whose cursor was exhausted (after_id 0xFFFFFFFF)    */
    uint32_t underfull_queries; /* of those, queries with fewer than k rows after their cursor           */
    uint64_t after_slots;       /* non-pad slots over all queries with a cursor                          */
} hvs_after_info;
int hvs_set_after(hvs_ctx *ctx, const float *after_dists /* host, nq */, const uint32_t *after_ids /* host, nq */, uint32_t nq);
int hvs_set_after_device(hvs_ctx *ctx, const float *d_after_dists /* device, nq */, const uint32_t *d_after_ids /* device, nq */, uint32_t nq,
                         void *stream);
int hvs_set_after_from_results(hvs_ctx *ctx);
int hvs_query_after(hvs_ctx *ctx, const float *q_rows, const float *after_dists, const uint32_t *after_ids, const float *max_d2 /* may be NULL */,
                    uint32_t nq, float sample_proportion, uint32_t *out_ids, float *out_dists);
int hvs_after_stats(hvs_ctx *ctx, hvs_after_info *out);
/* The host arithmetic of the contract for one query (no GPU, no context; any output may be NULL).  ids / dists: the query's m
 * matched keys in key order (full(q), or a prefix of it that reaches k keys past the cursor); pad_ids / pad_dists: the first k
 * padding rows and their exact-order distances (unused, may be NULL, when `padding` is 0).  out_ids / out_dists: the k slots of
 * the page behind the cursor -- the first k keys > (after_dist, after_id), then padding or empty slots, in (dist asc, id asc)
 * order; n_after: the non-pad slots. */
void hvs_after_plan(const uint32_t *ids, const float *dists, uint32_t m, uint32_t k, float after_dist, uint32_t after_id, const uint32_t *pad_ids,
                    const float *pad_dists, int padding, uint32_t *out_ids, float *out_dists, uint32_t *n_after);

/* ---- category sets: the k nearest rows whose C is in a per-query set ------------------------------ */

/*
 * "The k nearest rows whose category is one of s_1 .. s_m": a category set is a list of f32 values attached to one resident
 * query, given for all queries at once in CSR form -- set_offsets[nq + 1] (u32, ascending, set_offsets[0] == 0) and
 * set_values[set_offsets[nq]].
 *  - Types 1 and 3 with a non-empty set: the test `C == v` becomes "`C == s` for some s of the set"; the query's own v is
 *    ignored, the T window of type 3 stays.  A value is read as the engines read v (reference optimized_parallel.hpp:93-96: an
 *    int32 truncation, compared with C by IEEE ==): 5.9 names category 5, +0.0 and -0.0 one category; NaN and values outside
 *    the int32 range match nothing and are dropped; values that name the same category count once.
 *  - Any other query keeps its meaning: a query with an empty set, and a query of type 0, 2 or an invalid type whatever its set.
 *  - Everything else is the query's usual contract with the wider predicate: sampled prefix, live-row mask, caps, cursors, both
 *    distance orders, every k, the (dist asc, id asc) tie rule, padding from n-1, n-2, ... (or the last live ids) applied ONCE,
 *    0xFFFFFFFF / +inf in unmatched slots with hvs_set_padding(ctx, 0).  Ids and distance bits are those of a plain type-1/3
 *    query with v = v* on a copy of D in which every C of the set has been rewritten to a fresh value v*.  hvs_timing.pairs
 *    counts the rows that pass the set predicate in the prefix.
 *  - At most HVS_IN_MAX_VALUES distinct categories per query, and at most 2^32 - 1 sub-queries (below) in all: otherwise
 *    HVS_EINVAL and nothing changes, as for nq != the number of resident queries and for malformed offsets.
 * How: the index gives a query ONE position range of the (C,T) ordering, a set is a union of ranges.  So a query with m distinct
 * values is answered as m ordinary SUB-QUERIES over the same D with padding off, and one kernel merges their top-k lists by
 * key and pads once.  Rows of different categories are disjoint: the k smallest keys of the union of the lists are exactly
 * the set predicate's top-k.  The engines see the expanded query set -- nsub x (416 + 8k) bytes of queries and results beside
 * the user's -- and run exactly the kernels they run for plain queries.
 * Lifetime: sets belong to the resident query set as caps and cursors do: hvs_upload_queries, hvs_gen_queries,
 * hvs_set_queries_device, hvs_set_queries_from_rows and hvs_query remove them, and so does hvs_set_category_sets(ctx, NULL,
 * NULL, 0) (a no-op while none are attached).  Attaching or removing sets drops earlier results (as hvs_set_k does) and
 * removes caps and cursors: attach those afterwards, they stay one per USER query.  Every resident query index -- in
 * hvs_query_resident, hvs_download_results, hvs_export_results_device, hvs_download_queries (which keeps returning the user's
 * rows), hvs_set_max_dist2*, hvs_set_after* -- is the user's; hvs_set_after_from_results reads slot k-1 of the MERGED rows;
 * hvs_reserve(nq) sizes for the sub-queries of the first nq queries; hvs_last_timing reports the user's nq and a query_ms that
 * includes the merge; hvs_within_stats / hvs_after_stats follow the row-partitioned rules with "sub-query" for "part" (queries
 * the call's, under-full the merge's, slots summed over the sub-lists).  Only hvs_last_reruns speaks of the EXPANDED set: its
 * indices are sub-query indices.  hvs_query_resident resolves the sub-queries' filter re-runs before the merge is enqueued
 * (one host synchronisation, as on a row-partitioned context).  While no sets are attached every call runs exactly the
 * kernels, with exactly the arguments, it runs without these functions.
 * One GPU and replicated multi-GPU contexts (each GPU takes its owner range's slice of the CSR); a row-partitioned context
 * returns HVS_ESTATE, not supported (yet), and changes nothing; the D-sharded mode knows nothing of sets.  No data set loaded:
 * HVS_ESTATE.  The CSR is HOST memory; the queries themselves may have come from anywhere (the library reads their types back).
 *
 * hvs_query_in: hvs_upload_queries + hvs_set_category_sets + hvs_query_resident + hvs_download_results in one call.  It is NOT
 * the pipeline hvs_query is: the steps run one after the other.  Both set pointers NULL: exactly hvs_query.
 * hvs_in_stats: figures of the last call (after hvs_sync); HVS_ESTATE where hvs_last_timing has none to report; all zero when
 * the last call ran without sets.  Multi-GPU contexts: summed, max_set the largest, expand_ms / merge_ms the slowest GPU's.
 * hvs_in_plan: the host arithmetic (no GPU, no context; any output may be NULL).  q_rows (nq x 104, NULL = every query of type
 * 1) tells which queries test C.  A query without an effective set (empty set, or a type that does not test C) takes ONE
 * sub-query, itself; any other takes one per distinct category, values ascending, or one with value NaN (matches nothing)
 * when no value is left.  sub_offsets[nq + 1]; parent[nsub] and value[nsub]: sub-query j belongs to query parent[j] and
 * carries value[j] (a query without an effective set: its own v where q_rows is given, NaN otherwise).  Returns nsub, or
 * 0xFFFFFFFF (nothing written) for set_offsets[0] != 0, descending offsets, a set of more than HVS_IN_MAX_VALUES distinct
 * categories, or more than 2^32 - 2 sub-queries.
 */
#define HVS_IN_MAX_VALUES 64
typedef struct hvs_in_info {
    uint32_t set_queries;       /* queries of the last call that were answered through their set             */
    uint32_t sub_queries;       /* sub-queries the engines answered for the call's queries                   */
    uint32_t max_set;           /* most sub-queries of one query of the call                                 */
    uint32_t underfull_queries; /* queries with fewer than k keys in all their sub-lists together            */
    uint64_t merged_keys;       /* non-empty slots of the sub-lists the merge read                           */
    double   expand_ms;         /* device time of the expansion when the sets were attached                  */
    double   merge_ms;          /* device time of the call's merge kernel                                    */
} hvs_in_info;
int hvs_set_category_sets(hvs_ctx *ctx, const uint32_t *set_offsets /* host, nq+1 */, const float *set_values /* host */, uint32_t nq);
int hvs_query_in(hvs_ctx *ctx, const float *q_rows, const uint32_t *set_offsets, const float *set_values, uint32_t nq,
                 float sample_proportion, uint32_t *out_ids, float *out_dists);
int hvs_in_stats(hvs_ctx *ctx, hvs_in_info *out);
uint32_t hvs_in_plan(const float *q_rows /* nq x 104, may be NULL = all type 1 */, const uint32_t *set_offsets, const float *set_values, uint32_t nq,
                     uint32_t *sub_offsets /* nq+1 */, uint32_t *parent, float *value /* NaN-free but for "matches nothing"; both may be NULL */);

/* ---- category sets from device memory: the plan is made on the GPU --------------------------------- */

/*
 * hvs_set_category_sets_device(ctx, d_set_offsets, d_set_values, nq, stream): hvs_set_category_sets for a CSR that lies in
 * DEVICE memory -- a model's "allowed categories" per query, a join kernel's output.  Afterwards the context is in every respect
 * the context after hvs_set_category_sets of the same bytes: the same expanded resident set and answers, the same
 * hvs_download_queries, the same per-GPU slices on a replicated multi-GPU context, earlier results, caps and cursors dropped,
 * the same hvs_in_stats but for the two times, the same lifetime.  The call is accepted exactly when the host call accepts the
 * same bytes, and otherwise refused with HVS_EINVAL, nothing changing (sets already attached, results, caps and cursors stay in
 * force): d_set_offsets[0] != 0, a descending pair of offsets anywhere, a set of more than HVS_IN_MAX_VALUES distinct categories
 * on a query of any type, nq != the number of resident queries, 2^32 - 1 or more sub-queries counted as if every query tested
 * C (as hvs_in_plan(NULL, ...) counts them; the kernels form that sum and the true one in 64 bits).  Both pointers NULL, or
 * nq == 0: the sets are removed, as in the host call.  d_set_offsets == NULL with values given: HVS_EINVAL.  d_set_values ==
 * NULL is valid exactly when d_set_offsets[nq] == 0.  No data set loaded: HVS_ESTATE; a row-partitioned context: HVS_ESTATE,
 * not supported (yet).
 *
 * The buffers follow the rules of hvs_set_max_dist2_device / hvs_set_after_device: plain device memory of any visible GPU, both
 * on the same one; `stream` = the stream that produced them (NULL: the null stream); host memory of any kind is HVS_EINVAL with
 * the runtime's error cleared; the call blocks until the sets are attached; the buffers are only read -- offsets[nq] is trusted
 * to be the length of the value array once every pair of offsets has been found ascending, and nothing past it is read -- and
 * are the caller's again on return.
 *
 * What crosses PCIe: the set values never reach the host, and parent / value are never built there.  Three kernels make the
 * plan -- per query, one wave normalises its raw values (any number of them) and counts the distinct categories; a scan turns
 * the counts into sub_offsets; a second per-query pass writes parent and value, ascending --, bit for bit the plan of
 * hvs_in_plan(q_rows, ...).  The host reads back a status block (flags and the two 64-bit sub-query sums), the offsets at the
 * GPUs' slice boundaries (4 bytes per GPU, and offsets[nq]), and sub_offsets (4 bytes per user query) and one byte per query
 * "answered through its set", because hvs_query_resident maps query ranges to sub-query ranges on the host.  A buffer on the
 * context's own GPU is read in place; a GPU of a replicated context that does not hold the buffer copies its owner range's
 * slice of the offsets, and the values that slice points into, device to device.  Every GPU plans first and none changes
 * unless every plan is good: sets are attached on all GPUs or on none.
 * hvs_in_info.expand_ms of a device attach is the device time of the plan kernels plus the expansion.
 *
 * hvs_download_in_plan: a diagnostic -- the plan as it lies on the device (whichever entry point attached the sets) copied to
 * the host.  Returns nsub, the number of sub-queries; sub_offsets (nq + 1 entries of the USER's nq queries) is written whenever
 * it is not NULL, parent and value (nsub entries each) only when cap >= nsub.  Single-GPU contexts only (HVS_EINVAL otherwise);
 * HVS_ESTATE while no sets are attached.
 */
int hvs_set_category_sets_device(hvs_ctx *ctx, const uint32_t *d_set_offsets /* device, nq+1 */, const float *d_set_values /* device */,
                                 uint32_t nq, void *stream);
int hvs_download_in_plan(hvs_ctx *ctx, uint32_t *sub_offsets /* host, nuq+1, may be NULL */, uint32_t *parent,
                         float *value /* host, cap entries each, may be NULL */, uint32_t cap);

/* ---- per-query exclusion lists: the k nearest rows not in an id list -------------------------------- */
/*
 * An exclusion list is a set of row ids attached to ONE resident query: "not these rows" -- items already owned, everything shown
 * so far, the row the query was made from (hvs_set_queries_from_rows does not remove self-matches: a list of one id does).  The
 * lists of all resident queries are given at once in CSR form: excl_offsets[nq + 1] (u32, ascending, [0] == 0) and
 * excl_ids[excl_offsets[nq]] (u32).
 *
 * A row takes part in query q's answer only if it passes q's predicate (or its category set), lies in the sampled prefix, is
 * live, is within the cap if caps are set, is after the cursor if cursors are set, AND ITS ID IS NOT IN q's LIST.  Everything
 * else is as if the listed rows did not match: the slots they leave are filled by the usual padding rule (rows n-1, n-2, ... or
 * the last live ids; with hvs_set_padding(ctx, 0) they are empty, 0xFFFFFFFF / +inf).  Pad rows need not be outside the list,
 * as they need not pass the predicate or lie within a cap: a query whose list names a pad row may still be padded with it.
 * Ids, distance bits, the (dist asc, id asc) tie rule and hvs_timing.pairs do not change: `pairs` keeps counting
 * predicate-passing rows and does not look at lists.
 *
 * The law: with full(q) the matched keys of q in key order, the answer with padding off is the first k keys of full(q) whose id
 * is not listed, taken after cap and cursor, then empty slots.  Excluding the ids of pages 1..P of a query therefore gives
 * exactly page P+1 of a cursor walk -- ties and duplicate rows included, because the id decides.
 *
 * Ids.  An id is a row id of D as it is WHEN THE QUERY RUNS: a list is not a row reference.  An id that names no row -- >= n,
 * behind the sampled prefix, a dead row -- excludes nothing (an id >= n of today excludes the row an append gives that id).
 * 0xFFFFFFFF is ignored, so a result row with empty slots can be fed back as it is.  Duplicates and any order are fine.  No id
 * is validated and none can make the call fail: ids are only ever compared with row ids.
 *
 * Limits.  At most HVS_EXCLUDE_MAX raw entries per query (the offsets alone decide).  A longer list, offsets[0] != 0, a
 * descending pair of offsets, or nq != the number of resident queries: HVS_EINVAL, and nothing changes -- lists already attached,
 * results, caps and cursors stay in force.  No data loaded: HVS_ESTATE.
 *
 * Lifetime.  Lists belong to the resident query set exactly as caps and cursors do: every call that replaces the set removes
 * them (hvs_upload_queries, hvs_gen_queries, hvs_set_queries_device, hvs_set_queries_from_rows, hvs_query*), and so does
 * attaching or removing category sets.  Under category sets they stay one per USER query; each sub-query reads its parent's.
 * Both pointers NULL removes them.  Earlier results stay in place.  "No lists" is expressed by not setting them: while none are
 * set every call runs exactly the kernels it runs without this feature, with the same arguments.
 *
 * Lists compose with every engine, both distance orders, every k, caps, cursors (hvs_set_after_from_results included), the mask,
 * appended and updated rows, and category sets.  All three context kinds: a replicated context cuts the CSR by the owner
 * ranges; a row-partitioned one puts all lists on every part, each part keeping the ids of its row range as local ids (the last
 * part's range is open-ended).  The D-sharded recipe (sharding.py) knows nothing of lists.
 *
 * hvs_set_exclude_ids: from HOST memory.  hvs_set_exclude_ids_device: from DEVICE memory by the rules of hvs_set_after_device --
 * plain device memory of any visible GPU, both buffers on the same one; host memory of any kind is HVS_EINVAL with the runtime's
 * error cleared; the call blocks until the lists are attached.  It is accepted exactly when the host call accepts the same
 * bytes: a kernel checks the offsets and the host reads a status block back; offsets[nq] is trusted as the id array's length only
 * once every pair has been found ascending, and nothing past it is read.  Both entry points put the raw CSR on the device and
 * normalise it there (per list: drop 0xFFFFFFFF and, on a part, ids outside its rows; sort; drop duplicates), in place: the
 * list of query q starts at offsets[q].
 * hvs_query_excluding: hvs_query_after plus lists (host memory), sent whole before the pipeline starts; both list pointers NULL
 * is exactly hvs_query_after.
 * hvs_exclude_stats: figures of the last call.  excluding_queries: the call's queries while lists are set; kept_slots and
 * underfull_queries: from the final kernels, with the row-partitioned and sub-query rules of hvs_within_stats; refused_keys:
 * keys that reached an admission point and were dropped because they were listed -- a diagnostic whose exact value depends on
 * the thresholds of the run.  All zero for a call without lists.
 * hvs_download_exclude_plan: a diagnostic, single-GPU contexts only (HVS_EINVAL otherwise; HVS_ESTATE while no lists are
 * attached) -- the normalised lists as they lie on the device.  begin / count (nq entries each) are written when not NULL, ids
 * only when cap >= the id array's length, which is returned; entries of a list's raw extent behind its count are 0xFFFFFFFF.
 * hvs_exclude_plan: the arithmetic of the normalisation on the host, no GPU and no context: for rows [row0, row0 + n_rows) (a
 * single or replicated context: 0, 0xFFFFFFFF) writes begin[q] = offsets[q], count[q] and the normalised ids at
 * out_ids[begin[q] ..], the rest of the raw extent 0xFFFFFFFF; any output may be NULL, and with ids NULL only the offsets are
 * checked.  Returns the number of ids kept, or 0xFFFFFFFF for malformed offsets or an over-long list.  The device reproduces
 * it bit for bit.
 */
#define HVS_EXCLUDE_MAX 1024
typedef struct hvs_exclude_info {
    uint32_t excluding_queries;
    uint32_t underfull_queries;
    uint64_t kept_slots;
    uint64_t refused_keys;
} hvs_exclude_info;
int hvs_set_exclude_ids(hvs_ctx *ctx, const uint32_t *excl_offsets /* host, nq+1 */, const uint32_t *excl_ids /* host */, uint32_t nq);
int hvs_set_exclude_ids_device(hvs_ctx *ctx, const uint32_t *d_offsets /* device, nq+1 */, const uint32_t *d_ids /* device */, uint32_t nq,
                               void *stream);
int hvs_query_excluding(hvs_ctx *ctx, const float *q_rows, const uint32_t *excl_offsets, const uint32_t *excl_ids, const float *after_dists,
                        const uint32_t *after_ids, const float *max_d2 /* the last three may be NULL */, uint32_t nq, float sample_proportion,
                        uint32_t *out_ids, float *out_dists);
int hvs_exclude_stats(hvs_ctx *ctx, hvs_exclude_info *out);
int hvs_download_exclude_plan(hvs_ctx *ctx, uint32_t *begin, uint32_t *count /* host, nq each, may be NULL */, uint32_t *ids /* host, cap */,
                              uint32_t cap);
uint32_t hvs_exclude_plan(const uint32_t *offsets, const uint32_t *ids, uint32_t nq, uint32_t row0, uint32_t n_rows, uint32_t *begin,
                          uint32_t *count, uint32_t *out_ids);

/* ---- multi-vector queries: the k rows nearest to any of several vectors ----------------------------- */
/*
 * A user with three interests, an item with several embeddings, a text expanded into paraphrases: a query described by SEVERAL
 * vectors, asking for "the k rows that pass my predicate and are nearest to ANY of these vectors".  Extra vectors are attached
 * to the resident queries in CSR form: vec_offsets[nq + 1] (u32, ascending, [0] == 0) and vecs[vec_offsets[nq]][100] (f32).
 *
 * Definition.  User query q has the vector list V(q): its own 100 floats as vector 0, followed by its m(q) = vec_offsets[q + 1] -
 * vec_offsets[q] extras.  The key of a row for q is the SMALLEST key (distance bits, id) over the vectors of V(q), in the
 * engines' own key order (+inf after every finite value, the canonical NaN after +inf); each distance is the engine's
 * exact-order f32 distance to that one vector, bit for bit what a plain query with that vector reports.  The answer is the first
 * k rows in that key order among the rows that pass q's predicate, lie in the sampled prefix, are live, have `min distance <=
 * cap` if caps are set ("some vector within the cap") and are not in q's exclusion list.  Every id appears at most once among
 * the non-pad slots.  Then the usual padding (rows n-1, n-2, ... or the last live ids), a pad row reporting its smallest
 * distance over V(q); with hvs_set_padding(ctx, 0) the unmatched slots are 0xFFFFFFFF / +inf.  A query with m(q) == 0 is the
 * plain query: the same ids and distance bits as without the feature.
 *
 * How: q runs as 1 + m(q) ordinary SUB-QUERIES with padding off -- sub-query j is q's 104 floats with floats 4..103 replaced by
 * vector j -- on the expanded resident set that category sets use, and one kernel merges the sub-lists BY ID (per id the
 * smallest key), takes the k smallest and pads once.  That is exact: a row of the answer that attains its minimum at vector j
 * could only be missing from sub-list j if k rows had a smaller key under vector j, hence a smaller minimum key -- so every row
 * of the answer is in some sub-list with its true key, and a row outside the answer only ever shows a key at or above its true
 * one.
 *
 * Composes with every engine, both distance orders, every k, sample_proportion, padding on and off, caps, exclusion lists, the
 * live-row mask, appended and updated rows and compaction; caps and lists stay one per USER query, each sub-query reads its
 * parent's.  One GPU and replicated multi-GPU contexts (each GPU takes its owner range's slice of the CSR); a row-partitioned
 * context returns HVS_ESTATE and changes nothing.  The paging law of the exclusion lists holds: excluding the ids of pages 1..P
 * yields page P+1.
 * Does NOT compose, and says so:
 *  - cursors: a sub-query would test (d_j, id) > cursor per vector, and a row whose minimum key lies before the cursor would come
 *    back under another vector.  While vectors are attached hvs_set_after, hvs_set_after_device and hvs_set_after_from_results
 *    return HVS_ESTATE and change nothing (removing cursors, both pointers NULL, stays a no-op that succeeds).
 *  - category sets: there is one expanded set per context.  Attaching vectors removes category sets and attaching category sets
 *    removes vectors; the cross product is a later step.
 *
 * Lifetime: that of category sets.  Vectors belong to the resident query set: hvs_upload_queries, hvs_gen_queries,
 * hvs_set_queries_device, hvs_set_queries_from_rows and hvs_query* remove them, and so does hvs_set_query_vectors(ctx, NULL,
 * NULL, 0) (a no-op while none are attached).  Attaching or removing vectors drops earlier results and removes caps, cursors and
 * exclusion lists: attach those afterwards.  hvs_download_queries keeps returning the user's rows; hvs_reserve(nq) sizes for the
 * sub-queries; hvs_last_timing reports the user's nq and a query_ms that includes the merge; hvs_timing.pairs counts (vector,
 * row) pairs, the sub-queries' sum; hvs_last_reruns speaks sub-query indices; hvs_within_stats and hvs_exclude_stats follow the
 * sub-query rules they have under sets; hvs_in_stats reports zeros.  While no vectors are attached every call runs exactly the
 * kernels it runs without these functions, with exactly the same arguments.
 *
 * Limits.  At most HVS_VECTORS_MAX_EXTRA extras per query (64 sub-lists per merge), at most 2^32 - 2 sub-queries in all.  A
 * longer list, vec_offsets[0] != 0, a descending pair of offsets, or nq != the number of resident queries: HVS_EINVAL, and nothing
 * changes -- vectors already attached, results, caps and lists stay in force.  No data set loaded: HVS_ESTATE.  Vector components
 * are not validated: NaN and inf components give NaN or +inf distances, which sort by the key order as for a plain query.
 *
 * hvs_set_query_vectors: the CSR from HOST memory; both pointers NULL (or nq == 0) removes the vectors; vecs == NULL is valid
 * exactly when vec_offsets[nq] == 0.
 * hvs_set_query_vectors_device: the same from DEVICE memory by the rules of hvs_set_exclude_ids_device -- plain device memory of
 * any visible GPU, both buffers on the same one; host memory of any kind is HVS_EINVAL with the runtime's error cleared; the call
 * blocks until the vectors are attached.  It is accepted exactly when the host call accepts the same bytes: a kernel checks the
 * offsets and the host reads a status block back; offsets[nq] is trusted as the vector array's length only once every pair has
 * been found ascending, and nothing past it is read.  The vectors never cross PCIe; the host reads the offsets back (4 bytes per
 * query), because hvs_query_resident maps query ranges to sub-query ranges there.  The plan needs no scan: sub_off[q] =
 * offsets[q] + q.
 * hvs_query_vectors: hvs_upload_queries + hvs_set_query_vectors + hvs_query_resident + hvs_download_results in one call, the
 * steps one after the other (like hvs_query_in).  Both vector pointers NULL: exactly hvs_query.
 * hvs_vectors_stats: figures of the last call (after hvs_sync); HVS_ESTATE where hvs_last_timing has none to report; all zero when
 * the last call ran without vectors.  merged_keys: the non-empty slots of the sub-lists.  duplicate_keys: the keys the merge
 * dropped because its buffer held the same id with a key at least as small.  The merge streams the lists in order, 64 slots at a
 * time, through a buffer of CAP = 256 (k <= 128) or 512 keys; before a step that might not fit (held + 64 > CAP) it de-duplicates
 * the buffer and, if the step still might not fit, cuts it to the k smallest keys; it de-duplicates once more at the end.  A row
 * cut away and read again later therefore counts as new: duplicate_keys = merged_keys - distinct ids whenever no cut dropped a
 * row that returns (always when the lists' keys fit the buffer).  Multi-GPU contexts: counters summed, max_vectors the largest,
 * the two times the slowest GPU's.
 * hvs_vectors_plan: the merge's arithmetic for ONE query on the host, no GPU and no context: m unpadded lists of k slots each
 * (ids, dists: m x k, empty slots 0xFFFFFFFF / +inf), pad_ids / pad_dists (k each; the distances already the minimum over the
 * vectors; both may be NULL with padding == 0) and `padding`.  Writes the merged row (out_ids, out_dists: k slots; out_dists may
 * be NULL) and *n_duplicates (may be NULL) = non-empty slots - distinct ids, and returns the number of non-pad slots.
 * hvs_vectors_check: the offsets' arithmetic on the host: nsub = offsets[nq] + nq, or 0xFFFFFFFF for offsets == NULL, offsets[0] !=
 * 0, a descending pair, a list of more than HVS_VECTORS_MAX_EXTRA, or more than 2^32 - 2 sub-queries.  The device check
 * reproduces it.
 */
#define HVS_VECTORS_MAX_EXTRA 63
typedef struct hvs_vectors_info {
    uint32_t multi_queries;     /* queries of the last call with at least one extra vector                   */
    uint32_t sub_queries;       /* sub-queries the engines answered for the call's queries                   */
    uint32_t max_vectors;       /* most vectors (1 + extras) of one query of the call                        */
    uint32_t underfull_queries; /* queries with fewer than k distinct rows in all their sub-lists together   */
    uint64_t merged_keys;       /* non-empty slots of the sub-lists the merge read                           */
    uint64_t duplicate_keys;    /* ... of which dropped because the id was held with a key at least as small */
    double   expand_ms;         /* device time of the expansion when the vectors were attached               */
    double   merge_ms;          /* device time of the call's merge kernel                                    */
} hvs_vectors_info;
int hvs_set_query_vectors(hvs_ctx *ctx, const uint32_t *vec_offsets /* host, nq+1 */, const float *vecs /* host, x 100 */, uint32_t nq);
int hvs_set_query_vectors_device(hvs_ctx *ctx, const uint32_t *d_offsets /* device, nq+1 */, const float *d_vecs /* device, x 100 */,
                                 uint32_t nq, void *stream);
int hvs_query_vectors(hvs_ctx *ctx, const float *q_rows, const uint32_t *vec_offsets, const float *vecs, uint32_t nq,
                      float sample_proportion, uint32_t *out_ids, float *out_dists);
int hvs_vectors_stats(hvs_ctx *ctx, hvs_vectors_info *out);
uint32_t hvs_vectors_plan(const uint32_t *ids, const float *dists, uint32_t m, uint32_t k, const uint32_t *pad_ids,
                          const float *pad_dists, int padding, uint32_t *out_ids, float *out_dists, uint32_t *n_duplicates);
uint32_t hvs_vectors_check(const uint32_t *offsets, uint32_t nq);

/* ---- query clauses: the k nearest rows matching any of several clauses ------------------------------ */
/*
 * "C in {3, 7} and near any of my three interest vectors"; "T in last week OR in the same week last year"; "(C = 1 and T < t0)
 * or C = 2": a query that is an OR of CLAUSES, each a predicate [type, v, l, r] -- exactly the first four floats of a Q row --
 * plus, optionally, a vector of its own.  Extra clauses are attached to the resident queries in CSR form: clause_offsets[nq + 1]
 * (u32, ascending, [0] == 0), clause_attrs[clause_offsets[nq]][4] (f32) and clause_vecs, either NULL ("predicate-only clauses")
 * or [clause_offsets[nq]][100] (f32).
 *
 * Definition.  User query q has the clause list K(q): clause 0 is q's own row, its four attribute floats and its vector; then
 * come its m(q) = clause_offsets[q + 1] - clause_offsets[q] extras, extra j with attributes clause_attrs[j] and the vector
 * clause_vecs[j], or q's own vector when clause_vecs == NULL.  A row PASSES clause c if it passes c's predicate exactly as a plain
 * query with those four floats would (an invalid type keeps whatever meaning it has for a plain query).  The key of a row for q
 * is the SMALLEST key (distance bits, id) over the clauses it passes, in the engines' own key order; each distance is the
 * engine's exact-order f32 distance to that clause's vector.  The answer is the first k rows in key order among the rows that
 * pass at least one clause, lie in the sampled prefix, are live, have `min key's distance <= cap` if caps are set, are not in
 * q's exclusion list and, where cursors are allowed (below), have a key strictly after the cursor.  Every id appears at most once
 * among the non-pad slots.  The usual padding is applied ONCE, a pad row reporting its smallest distance over the vectors of
 * K(q); with hvs_set_padding(ctx, 0) the unmatched slots are 0xFFFFFFFF / +inf.  A query with m(q) == 0 is the plain query, bit
 * for bit.
 *
 * How: q runs as 1 + m(q) ordinary SUB-QUERIES with padding off on the expanded resident set that category sets and extra vectors
 * use (its third client), and one kernel merges the sub-lists by id.  Exact by the argument of the multi-vector queries with
 * "vector j" read as "clause j": a row of the answer that attains its minimum at clause j is in sub-list j -- otherwise k rows
 * passing clause j would have smaller keys, hence smaller minimum keys --, and a row outside the answer only ever shows a key at
 * or above its true one.  The merged row's arithmetic for one query is hvs_vectors_plan's: the smallest key per id,
 * the k smallest, pad once; there is no second copy of it.
 *
 * hvs_timing.pairs counts (clause, row) pairs, the sub-queries' sum: a row passing two clauses counts twice.
 *
 * Cursors.  With predicate-only clauses every row has ONE key whichever clause admits it, so each sub-query applies the cursor
 * itself and the merge by id drops the equal duplicates: hvs_set_after, hvs_set_after_device and hvs_set_after_from_results work
 * (the last one reads the merged rows), and the paging law of the cursors holds.  With clause_vecs != NULL (and at least one extra
 * clause in the whole CSR: without any, the pointer means nothing) they return HVS_ESTATE and change nothing, for the reason given for extra vectors; paging goes through exclusion lists there.
 *
 * Composes with every engine, both distance orders, every k, sample_proportion, padding on and off, caps, exclusion lists, the
 * live-row mask, appended and updated rows and compaction; caps, cursors and lists stay one per USER query, each sub-query reads
 * its parent's.  One GPU and replicated multi-GPU contexts (each GPU takes its owner range's slice of the CSR; attached on all
 * GPUs or on none); a row-partitioned context returns HVS_ESTATE and changes nothing.
 *
 * Lifetime: that of extra vectors.  There is one expanded set per context: attaching clauses replaces category sets or vectors,
 * attaching category sets or vectors replaces clauses, and removing one client is a no-op while another is attached.  Clauses
 * belong to the resident query set: hvs_upload_queries, hvs_gen_queries, hvs_set_queries_device, hvs_set_queries_from_rows and
 * hvs_query* remove them, and so does hvs_set_query_clauses(ctx, NULL, NULL, NULL, 0).  Attaching or removing clauses drops
 * earlier results and removes caps, cursors and exclusion lists: attach those afterwards.  hvs_download_queries keeps returning
 * the user's rows; hvs_reserve(nq) sizes for the sub-queries; hvs_last_timing reports the user's nq and a query_ms that includes
 * the merge; hvs_last_reruns speaks sub-query indices; hvs_in_stats and hvs_vectors_stats report zeros after a clause call.  While
 * no clauses are attached every call runs exactly the kernels it runs without these functions, with exactly the same arguments.
 *
 * Limits.  At most HVS_CLAUSES_MAX_EXTRA extras per query (256 lists per merge), at most 2^32 - 2 sub-queries in all.  A longer
 * list, clause_offsets[0] != 0, a descending pair of offsets, nq != the number of resident queries, or clause_attrs == NULL while
 * clause_offsets[nq] > 0: HVS_EINVAL, and nothing changes -- clauses already attached, results, caps, cursors and lists stay in
 * force.  No data set loaded: HVS_ESTATE.  Attribute and vector values are not validated.
 *
 * hvs_set_query_clauses: the CSR from HOST memory; all pointers NULL (or nq == 0) removes the clauses.
 * hvs_set_query_clauses_device: the same from DEVICE memory by the rules of hvs_set_query_vectors_device -- plain device memory of
 * any visible GPU, all buffers on the same one; host memory of any kind is HVS_EINVAL with the runtime's error cleared; the call
 * blocks until the clauses are attached.  It is accepted exactly when the host call accepts the same bytes.  Attributes and
 * vectors never cross PCIe: the host reads back the status block and the offsets only.
 * hvs_query_clauses: hvs_upload_queries + hvs_set_query_clauses + hvs_query_resident + hvs_download_results in one call, the steps
 * one after the other.  All clause pointers NULL: exactly hvs_query.
 * hvs_clauses_stats: figures of the last call (after hvs_sync); HVS_ESTATE where hvs_last_timing has none to report; all zero when
 * the last call ran without clauses.  The merge streams a query's lists in sub-query order, 64 slots (a CHUNK) at a time, through a
 * buffer of CAP = 256 (k <= 128) or 512 keys.  Before a chunk that might not fit (held + 64 > CAP) it de-duplicates the buffer by
 * id and, if the chunk still might not fit, CUTS it to the k smallest keys; the largest key kept becomes the threshold.  A loaded
 * key is admitted only if it is strictly below the threshold, and after a chunk in which some slot was empty or not below the
 * threshold the rest of that list is not loaded (lists ascend).  It de-duplicates once more at the end.  read_keys: the non-empty
 * slots loaded.  duplicate_keys: keys a de-duplication dropped.  bounded_keys: keys loaded and not admitted.  skipped_chunks:
 * chunks never loaded.  Multi-GPU contexts: counters summed, max_clauses the largest, the two times the slowest GPU's.
 * hvs_clauses_check: the offsets' arithmetic on the host, no GPU: nsub = offsets[nq] + nq, or 0xFFFFFFFF for offsets == NULL,
 * offsets[0] != 0, a descending pair, a list of more than HVS_CLAUSES_MAX_EXTRA, or more than 2^32 - 2 sub-queries.  The device
 * check reproduces it.
 */
#define HVS_CLAUSES_MAX_EXTRA 255
typedef struct hvs_clauses_info {
    uint32_t clause_queries;    /* queries of the last call with at least one extra clause                    */
    uint32_t sub_queries;       /* sub-queries the engines answered for the call's queries                    */
    uint32_t max_clauses;       /* most clauses (1 + extras) of one query of the call                         */
    uint32_t underfull_queries; /* queries with fewer than k distinct rows in all their sub-lists together    */
    uint64_t read_keys;         /* non-empty slots the merge loaded                                           */
    uint64_t duplicate_keys;    /* keys dropped at a de-duplication                                           */
    uint64_t bounded_keys;      /* keys loaded and not admitted because they were not below the threshold     */
    uint64_t skipped_chunks;    /* 64-slot chunks never loaded                                                */
    double   expand_ms;         /* device time of the expansion when the clauses were attached                */
    double   merge_ms;          /* device time of the call's merge kernel                                     */
} hvs_clauses_info;
int hvs_set_query_clauses(hvs_ctx *ctx, const uint32_t *clause_offsets /* host, nq+1 */, const float *clause_attrs /* host, x 4 */,
                          const float *clause_vecs /* host, x 100, may be NULL */, uint32_t nq);
int hvs_set_query_clauses_device(hvs_ctx *ctx, const uint32_t *d_offsets /* device, nq+1 */, const float *d_attrs /* device, x 4 */,
                                 const float *d_vecs /* device, x 100, may be NULL */, uint32_t nq, void *stream);
int hvs_query_clauses(hvs_ctx *ctx, const float *q_rows, const uint32_t *clause_offsets, const float *clause_attrs,
                      const float *clause_vecs, uint32_t nq, float sample_proportion, uint32_t *out_ids, float *out_dists);
int hvs_clauses_stats(hvs_ctx *ctx, hvs_clauses_info *out);
uint32_t hvs_clauses_check(const uint32_t *offsets, uint32_t nq);

/* ---- per-query candidate lists: the k nearest rows among an id list --------------------------------- */
/*
 * A candidate list is a set of row ids attached to ONE resident query: "search only among THESE rows" -- the hits of a keyword
 * stage to be re-ranked, a user's saved items, the rows an access-control list admits.  The lists of all resident queries are
 * given at once in CSR form: cand_offsets[nq + 1] (u32, ascending, [0] == 0) and cand_ids[cand_offsets[nq]] (u32).
 *
 * A row takes part in query q's answer only if ITS ID IS IN q's LIST and it also passes q's predicate (as a plain query reads
 * the four attribute floats; an invalid type matches nothing), lies in the sampled prefix, is live, is within the cap if caps
 * are set, is after the cursor if cursors are set, and is not in q's exclusion list if exclusion lists are set.
 *
 * The law: with full(q) the matched keys of q in key order, the answer with padding off is the first k keys of full(q) whose id
 * is listed, taken after cap, exclusion and cursor, then empty slots (0xFFFFFFFF / +inf).  With padding on the usual rule fills
 * the rest ONCE: rows n-1, n-2, ..., or the last live ids under a mask; pad rows need not be listed.  Ids, distance bits (the
 * engines' exact-order function in the context's distance order) and the (dist asc, id asc) tie rule are those of every other
 * call.  AN EMPTY LIST MATCHES NOTHING; "no restriction" is expressed by attaching no lists.
 *
 * Ids.  The rules of exclusion lists: an id is a row id of D as it is WHEN THE QUERY RUNS; an id that names no row -- >= n,
 * behind the sampled prefix, a dead row -- contributes nothing; 0xFFFFFFFF is ignored, so a result row with empty slots can be
 * fed in as it is; duplicates count once; any order is fine.  Nothing is validated beyond the offsets: no id can make a call
 * fail, and none is used as an index unchecked.
 *
 * Limits.  At most HVS_CANDIDATES_MAX raw entries per query (the offsets alone decide).  A longer list, offsets[0] != 0, a
 * descending pair of offsets, nq != the number of resident queries, or cand_ids == NULL with offsets[nq] > 0: HVS_EINVAL, and
 * nothing changes -- lists already attached, results, caps and cursors stay in force.  No data loaded: HVS_ESTATE.  Both
 * pointers NULL removes the lists.
 *
 * Lifetime.  That of exclusion lists: every call that replaces the resident set removes them, and so does attaching or removing
 * category sets, query vectors or clauses.  Earlier results stay in place.  While no lists are attached every call runs exactly
 * the kernels it runs without this feature, with the same arguments.
 *
 * Composes with every k, both distance orders, the padding setting, sample_proportion, caps, cursors (hvs_set_after_from_results
 * included), exclusion lists, the mask, appended rows, updated rows and compaction: the scan reads D as it is, so nothing is
 * stale and no tail exists for it.  hvs_set_engine has no effect on such a call: there is one way to answer it, a gather of the
 * listed rows (hvs_timing.engine reports HVS_ENGINE_EXACT_SCAN).  Does NOT compose (yet) with the expanded resident set: while
 * category sets, query vectors or clauses are attached hvs_set_candidate_ids* returns HVS_ESTATE and nothing changes.
 * All three context kinds: a replicated context cuts the CSR by the owner ranges; a row-partitioned one puts all lists on every
 * part, each part keeping the ids of its row window as local ids (the last part's window is open-ended) and answering with
 * padding off; the merge of the parts pads.
 *
 * hvs_set_candidate_ids: from HOST memory.  hvs_set_candidate_ids_device: from DEVICE memory by the rules of
 * hvs_set_exclude_ids_device; it is accepted exactly when the host call accepts the same bytes.
 * hvs_query_among: upload + attach (max_d2, may be NULL: caps) + resident run + download; it is not a pipeline.
 * hvs_candidates_stats: figures of the last call, all zero for a call without lists.  listed_queries: the call's queries;
 * scanned_ids: the normalised entries of their lists; passing_ids: distinct listed rows in the prefix that are live and pass
 * the predicate; kept_slots and underfull_queries: non-pad slots written and queries with fewer than k of them (row-partitioned:
 * the rules of hvs_exclude_stats); scan_ms: device time of the scan kernel.  hvs_last_timing after such a call reports
 * pairs = passing_ids, scanned_pairs = scanned_ids, rescored_pairs = retry_queries = fallback_queries = 0 and main_kernel_ms =
 * the scan kernel's.  hvs_within_stats, hvs_after_stats and hvs_exclude_stats report the kept slots and under-full queries of
 * such a call where their feature is attached; exhausted cursors and refused keys are not counted by it.
 * hvs_download_candidates_plan: the diagnostic twin of hvs_download_exclude_plan, single-GPU contexts only.
 * hvs_candidates_plan: the arithmetic of the normalisation on the host, no GPU and no context; layout and return convention are
 * those of hvs_exclude_plan, the limit is HVS_CANDIDATES_MAX.  The device reproduces it bit for bit.
 */
#define HVS_CANDIDATES_MAX 8192
typedef struct hvs_candidates_info {
    uint32_t listed_queries;
    uint32_t underfull_queries;
    uint64_t scanned_ids;
    uint64_t passing_ids;
    uint64_t kept_slots;
    double scan_ms;
} hvs_candidates_info;
int hvs_set_candidate_ids(hvs_ctx *ctx, const uint32_t *cand_offsets /* host, nq+1 */, const uint32_t *cand_ids /* host */, uint32_t nq);
int hvs_set_candidate_ids_device(hvs_ctx *ctx, const uint32_t *d_offsets /* device, nq+1 */, const uint32_t *d_ids /* device */, uint32_t nq,
                                 void *stream);
int hvs_query_among(hvs_ctx *ctx, const float *q_rows, const uint32_t *cand_offsets, const uint32_t *cand_ids,
                    const float *max_d2 /* may be NULL */, uint32_t nq, float sample_proportion, uint32_t *out_ids, float *out_dists);
int hvs_candidates_stats(hvs_ctx *ctx, hvs_candidates_info *out);
int hvs_download_candidates_plan(hvs_ctx *ctx, uint32_t *begin, uint32_t *count /* host, nq each, may be NULL */, uint32_t *ids /* host, cap */,
                                 uint32_t cap);
uint32_t hvs_candidates_plan(const uint32_t *offsets, const uint32_t *ids, uint32_t nq, uint32_t row0, uint32_t n_rows, uint32_t *begin,
                             uint32_t *count, uint32_t *out_ids);

/* ---- shared row sets: the k nearest rows inside a per-query bitmap ---------------------------------- */
/*
 * A row set is a bitmap over the rows of D that MANY queries share: the rows a tenant owns, the rows an access-control group may
 * read.  The sets belong to the DATA SET: a context holds n_sets of them, 1 <= n_sets <= HVS_ROW_SETS_MAX, each in the layout
 * of hvs_set_row_mask's live_bits -- ceil(n / 64) u64 words, row i at bit i & 63 of word i >> 6 -- one after the other.  Bits at
 * or past n are ignored on input and read back clear.  The set INDICES belong to the RESIDENT QUERIES: one uint32_t per query, a
 * set index < n_sets, or 0xFFFFFFFF for "no restriction".
 *
 * The law is that of exclusion lists with one clause swapped: a row takes part in query q's answer only if it passes every other
 * test -- predicate, sampled prefix, live, cap, cursor, exclusion list, candidate list -- AND ITS BIT IS SET IN q's SET.  With
 * padding off the answer is the first k keys of full(q) whose row is in the set, taken after cap, cursor and exclusion list (under
 * a candidate list only the listed rows count), then empty slots (0xFFFFFFFF / +inf).  With padding on the usual rule fills the
 * rest ONCE; pad rows need not be in the set.  Ids, distance bits, the (dist asc, id asc) tie rule, the sampled prefix and
 * hvs_timing.pairs are unchanged: pairs do not look at sets, as they do not look at lists.  A query with 0xFFFFFFFF keeps its
 * meaning; AN EMPTY SET MATCHES NOTHING.
 *
 * hvs_set_row_sets: n_sets bitmaps from HOST memory (bits == NULL: n_sets empty sets); n_sets == 0 removes the sets.  Replacing
 * or removing the sets removes every query's index and drops the results.  n_sets > HVS_ROW_SETS_MAX, or sets of more than
 * 2^32 - 1 u32 words altogether: HVS_EINVAL, and nothing changes.  No data loaded: HVS_ESTATE.
 * hvs_set_row_sets_device: the same from DEVICE memory of one GPU, complete on `stream` (the rules of
 * hvs_set_exclude_ids_device); a pointer that is not device memory: HVS_EINVAL.
 * hvs_assign_row_sets: sets (member != 0) or clears the bits of ONE set for the rows named by a host id list, with atomicOr /
 * atomicAnd on the device.  Ids >= n (0xFFFFFFFF among them) are ignored.  This is how appended rows get into a set, and how sets
 * are built from a tenant-to-ids CSR.  set >= n_sets: HVS_EINVAL; no sets loaded: HVS_ESTATE.  Results of earlier calls stay.
 * hvs_get_row_sets: the sets as they are, n_sets x ceil(n / 64) words to host memory.
 * hvs_set_query_row_sets: one index per resident query from HOST memory; NULL removes the indices.  An index >= n_sets other than
 * 0xFFFFFFFF, or nq != the number of resident queries: HVS_EINVAL; no sets loaded: HVS_ESTATE; either way nothing changes --
 * indices already attached, sets, results, caps, cursors and lists stay in force.
 * hvs_set_query_row_sets_device: from DEVICE memory; it is accepted exactly when the host call accepts the same bytes (a check
 * kernel writes a status block on every GPU, and the host judges all of them before any GPU commits).
 * hvs_query_in_row_sets: upload + attach + resident run + download; it is not a pipeline.
 *
 * Lifetime.  The BITMAPS survive new queries, hvs_set_k, an engine change, hvs_delete_rows, hvs_set_row_mask, hvs_update_rows and
 * hvs_reindex: an id keeps its bits.  hvs_append_rows gives the new rows clear bits in every set (the bitmaps are sized for the
 * capacity of D and re-strided when it grows); hvs_trim_rows shrinks them; hvs_compact renumbers them on the device exactly as
 * hvs_row_sets_compact_plan does; hvs_load_data*, hvs_gen_data drop them.  The INDICES have the lifetime of exclusion lists:
 * every call that replaces the resident set removes them, and so does attaching or removing category sets, query vectors or
 * clauses; attached after those, every sub-query takes its parent's index.  While no indices are attached every call runs exactly
 * the kernels it runs without this feature, with the same arguments.
 *
 * Composes with every engine and k, both distance orders, the padding setting, sample_proportion, caps, cursors, exclusion
 * lists, candidate lists, the expanded resident set, the mask, appended and updated rows, and compaction.  All three context
 * kinds: a replicated context holds all bitmaps on every GPU and cuts the indices by the owner ranges; a row-partitioned one
 * holds the WHOLE bitmaps on every part, which tests bit (first row of the part + local id), answers with padding off and leaves
 * the padding to the merge of the parts.  A row-partitioned context has no row-set operations, so hvs_assign_row_sets is the only
 * mutation there; it goes to every part.
 *
 * hvs_row_sets_stats: n_sets, words_per_set (u64 words) and bytes (device memory of one GPU) of the sets loaded; and of the last
 * call, all zero for a call without indices: restricted_queries (queries answered whose index is not 0xFFFFFFFF; under the
 * expanded set counted per sub-query, as the slots are), refused_keys (keys that every other test admitted and the set refused,
 * at any admission point: a lower bound is the number of such keys in front of the k-th kept one; for the thresholds of the run
 * the exact value is pinned by the host model of tests/selectivity_model.py, "Row sets", which tests/test_filter_selectivity.py
 * asserts equal on every filter engine -- a key that is listed AND outside the set counts for the list alone), kept_slots (non-pad slots
 * written) and underfull_queries (queries with fewer than k of them; row-partitioned: the rules of hvs_exclude_stats).  Keys
 * refused by a set and keys refused by an exclusion list are counted apart: hvs_exclude_stats reports what it reported before.
 * hvs_row_sets_compact_plan: pure host arithmetic, no GPU and no context: the sets as they must be after hvs_compact under the
 * mask live_bits (NULL: every row live), out[s][j] = bits[s][id of the j-th live row], in the layout of the input (n_sets x
 * ceil(n / 64) words; bits at or past the number of live rows clear).  The device reproduces it bit for bit.
 */
#define HVS_ROW_SETS_MAX 256
typedef struct hvs_row_sets_info {
    uint32_t n_sets;
    uint32_t words_per_set;
    uint64_t bytes;
    uint32_t restricted_queries;
    uint32_t underfull_queries;
    uint64_t refused_keys;
    uint64_t kept_slots;
} hvs_row_sets_info;
int hvs_set_row_sets(hvs_ctx *ctx, const uint64_t *bits /* host, n_sets x ceil(n/64), or NULL = all sets empty */, uint32_t n_sets);
int hvs_set_row_sets_device(hvs_ctx *ctx, const uint64_t *d_bits /* device, or NULL */, uint32_t n_sets, void *stream);
int hvs_assign_row_sets(hvs_ctx *ctx, uint32_t set, const uint32_t *ids /* host */, uint32_t count, int member);
int hvs_get_row_sets(hvs_ctx *ctx, uint64_t *bits /* host, n_sets x ceil(n/64) */);
int hvs_set_query_row_sets(hvs_ctx *ctx, const uint32_t *set_of_query /* host, nq, or NULL */, uint32_t nq);
int hvs_set_query_row_sets_device(hvs_ctx *ctx, const uint32_t *d_set_of_query /* device, nq, or NULL */, uint32_t nq, void *stream);
int hvs_query_in_row_sets(hvs_ctx *ctx, const float *q_rows, const uint32_t *set_of_query, uint32_t nq, float sample_proportion,
                          uint32_t *out_ids, float *out_dists);
int hvs_row_sets_stats(hvs_ctx *ctx, hvs_row_sets_info *out);
void hvs_row_sets_compact_plan(const uint64_t *bits, const uint64_t *live_bits /* may be NULL */, uint32_t n, uint32_t n_sets,
                               uint64_t *out_bits);

#ifdef __cplusplus
}
#endif
#endif /* HVS_H */
