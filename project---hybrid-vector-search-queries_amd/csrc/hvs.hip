// hvs.hip -- host side of libhvs.so: context, HBM residency, launch plan, C ABI (include/hvs.h).
//
// Build (see __graft_entry__.build):
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared hvs.hip -o libhvs.so
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <functional>
#include <iterator>
#include <new>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include <sched.h>

#include <rocprim/rocprim.hpp>

#include "../../include/hvs.h"
#include "hvs_kernels.h"
#include "hvs_filter.h"

namespace {

thread_local std::string g_global_err;
int fail(hvs_ctx* c, int code, const std::string& msg);  // (defined below, with staging_copy: the state structs call them)
void staging_copy(void* dst, const void* src, size_t bytes);
struct ExpandedKind;  // (what tells the clients of the expanded resident set apart: below, with in_commit)
#define HVS_HIP(ctx, call)                                                                                    \
    do {                                                                                                       \
        hipError_t e_ = (call);                                                                                \
        if (e_ != hipSuccess)                                                                                  \
            return fail(ctx, e_ == hipErrorOutOfMemory ? HVS_ENOMEM : HVS_EHIP,                                \
                        std::string(#call) + ": " + hipGetErrorString(e_));                                    \
    } while (0)

}  // namespace

// The index's per-ordering buffers: rows sorted by (C,T) or by T alone
struct HvsOrdering {
    uint64_t* keys = nullptr;  // sorted attribute keys
    uint32_t* perm = nullptr;  // position -> original row id
    uint4* tiles = nullptr;    // A-operand tiles (16-bit or INT8), level-interleaved
    uint4* nrm = nullptr;      // INT8 formats: the tiles' side data (accumulator inits; 32x32x32: + dims 96..99)
    uint32_t* bpos = nullptr;  // storage index -> block
    // (not part of the index: sized by n alone, kept across free_index and freed with the context)
    uint32_t* lp = nullptr;    // live rows in front of each position (hvs_k_live_flags), [n + 1]
};

// What the host needs to know of a tile format (HVS_FMT_*), in one place
typedef void (*HvsFilterKernel)(const uint4*, const uint4*, const uint4*, const uint4*, const uint32_t*, const uint32_t*, HvsLevels, uint32_t,
                                HvsBatch, HvsItems, unsigned long long*);
typedef void (*HvsBuildI8Kernel)(const float*, uint32_t, const uint32_t*, HvsLevels, const HvsQuant*, uint4*, int*, uint32_t*, HvsBounds*);
struct HvsHostFmt {
    size_t tile_u4, nrm_u4;     // uint4 per 32-row tile: operands, side data (0: none)
    HvsBuildI8Kernel build_i8;  // the INT8 formats' builder (null: hvs_k_build_tiles, which takes the 16-bit format as an argument)
    HvsFilterKernel filter;
};
static HvsHostFmt hvs_host_fmt(int fmt, bool rotated)
{
    switch (fmt) {
    case HVS_FMT_I8X16:
        return {HVS_I8X16_TILE_U4, HVS_I8X16_NRM_U4, rotated ? hvs_k_build_tiles_i8x16_rot : hvs_k_build_tiles_i8x16, hvs_k_filter_i8x16};
    case HVS_FMT_I8: return {HVS_I8_TILE_U4, HVS_I8_NRM_U4, hvs_k_build_tiles_i8, hvs_k_filter_mfma<HVS_FMT_I8>};
    case HVS_FMT_F16: return {HVS_TILE_U4, 0, nullptr, hvs_k_filter_mfma<HVS_FMT_F16>};
    default: return {HVS_TILE_U4, 0, nullptr, hvs_k_filter_mfma<HVS_FMT_BF16>};
    }
}
// The error bound needs finite row norms: data with inf/NaN components (or |d|^2 overflowing f32) is answered by the
// exact engine only
static bool hvs_bounds_usable(int fmt, const HvsBounds& hb)
{
    if (HVS_IS_I8(fmt)) return std::isfinite(hb.e_d8) && std::isfinite(hb.n_d8) && hb.n_d8 < 1.0e15f;
    const bool finite = std::isfinite(hb.e_d) && std::isfinite(hb.nb_d) && std::isfinite(hb.hmax) && std::isfinite(hb.rho);
    // FP16: every component and the three pieces of -|d|^2/2 inside the half-precision range (denormal flushing is part of
    // the bound: HVS_F16_FLUSH)
    if (fmt == HVS_FMT_F16) return finite && hb.hmax < 6.0e4f;
    // (norms near the f32 denormal range: BF16 operands might be flushed by the matrix pipe, which the
    // error bound does not model)
    return finite && !(hb.hmax > 1.0e30f) && !(hb.hmax > 0.0f && hb.hmax < 1.0e-20f);
}

// Tile-format state of one data set's index: what is built, what the planner decided, what was rejected
struct HvsFormatState {
    int built = HVS_FMT_NONE;   // format of the tiles both orderings carry (HVS_FMT_NONE: no usable tiles)
    bool built_rot = false;     // ... INT8 tiles, cut from the rotated vectors
    int planned = HVS_FMT_BF16; // what HVS_ENGINE_AUTO uses for this data set (HVS_FMT_NONE: no filter beats the exact engine)
    bool i8_usable = false;     // the INT8 quantiser has a finite, non-zero spread to work with
    bool i8_rot = false;        // the INT8 centre / scale (d_quant) live in the rotated space (HvsQuant::rot): the next INT8 build is rotated
    bool i8_rejected = false;   // the INT8 tiles were built and their bound was unusable: do not try again
    bool f16_rejected = false;  // likewise the FP16 tiles (components beyond the half-precision range)
};

// Row-set state of one data set: which rows are live and which of them the index is right about -- all that
// deletion, append, update and compaction maintain beside hvs_ctx's d_data, n, n_indexed and have_order.  The invariants:
//   - h_live.empty()  <=>  no mask set: every row live, n_dead == 0, and no launch reads d_live, d_pad_ids or d_mask_stat
//   - d_live, once allocated, has room for n_cap rows (live_cap >= ceil(n_cap / 64)); the first mask call after a reset makes it
//   - h_stale is ascending, unique, below n_indexed, and mirrored in d_stale_ids[0 .. h_stale.size())
//   - d_ilive is valid  <=>  !h_stale.empty(); while it is, n_indexed does not change
struct HvsRowSet {
    // -- live-row mask.  While nothing is masked (masked()) every launch takes its kernel's unmasked instantiation
    std::vector<uint64_t> h_live;   // host copy: ceil(n / 64) words, bits past n clear
    uint32_t* d_live = nullptr;     // the same bits as u32 words in HBM
    uint32_t n_dead = 0, live_cap = 0;  // dead rows; u64 words d_live has room for
    uint32_t* d_pad_ids = nullptr;  // the last k live ids in descending order (HVS_KMAX entries)
    unsigned long long* d_mask_stat = nullptr;  // [0]: rows whose tile entry carries the never-hit encoding, both orderings
    bool lp_valid = false;          // HvsOrdering::lp holds the counts of the current mask and stale set
    bool cut_valid = false;         // cut id of the sampled live prefix for sample_proportion cut_sp (hvs_mask_plan), cached
    float cut_sp = 0.0f;
    uint32_t cut_id = 0, cut_sn_live = 0;
    // -- capacity and tail: ids [n_indexed, n), scanned exactly by hvs_k_scan_tail for every batch that goes through the index
    uint32_t n_cap = 0;             // rows d_data has room for (hvs_reserve_rows / geometric growth of hvs_append_rows)
    uint32_t tail_limit = 0;        // hvs_set_tail_limit (0: the default rule, tail_limit_of); a setting, kept by every reset
    uint32_t reindexes = 0;         // index builds caused by appends, updates, compactions or hvs_reindex since the last load
    double reindex_ms = 0.0;        // the last of them
    uint32_t index_tried_n = 0;     // no-index state: n at the last attempt to build one (0: none yet)
    // -- stale set.  An indexed row whose contents changed is STALE: alive in D, dead as far as the index knows.
    // While there are such rows the launches that reach a row THROUGH THE INDEX take d_ilive (index_mask()), every masked kernel
    // runs in its MASKED form, and hvs_k_scan_stale scans the stale rows by id.  Empty list: none of the buffers is read.
    std::vector<uint32_t> h_stale;
    uint32_t* d_stale_ids = nullptr;
    // two planes of W = 2 ceil(n_indexed / 64) u32 words: [0, W) live AND NOT stale, [W, 2W) the row mask's bits of the
    // indexed rows (what hvs_k_rescore tells stale from dead by, HVS_RESCORE_TWO_MASKS)
    uint32_t* d_ilive = nullptr;
    uint32_t stale_cap = 0, ilive_cap = 0;  // ids d_stale_ids / u32 words d_ilive has room for
    // -- staging, kept between calls: hvs_delete_rows' id list; hvs_update_rows' rows, ids and the staged row of each id.  Per-call
    // buffers, freed when the call ends (free_call_scratch): hvs_compact's bounce buffer and rank table, hvs_trim_rows' smaller D
    uint32_t *d_mask_ids = nullptr, *d_upd_ids = nullptr, *d_upd_from = nullptr;
    float* d_upd_rows = nullptr;
    uint32_t mask_ids_cap = 0, upd_cap = 0;
    uint2* d_cmp_bounce = nullptr;
    uint32_t* d_cmp_rank = nullptr;
    float* d_trim = nullptr;
    hvs_compact_info cstat{};       // figures of the last hvs_compact since the last load
    // -- shared row sets: n_sets bitmaps in d_sets, sets_words u32 words each (an even number: whole u64 words of
    // the contract's layout), one bit per row.  While n_sets == 0 nothing here is read.  The invariants:
    //   - sets_words >= 2 ceil(max(n_cap, rows) / 64), so every row D has room for has a word in every set
    //   - the bits at or past the rows the sets cover (set_rows(): n, or the whole D's rows on a part of a row-partitioned
    //     context, whose ids start at sets_row0) are clear: an appended row is in no set
    uint32_t* d_sets = nullptr;
    uint32_t n_sets = 0, sets_words = 0;
    uint32_t sets_part_rows = 0, sets_row0 = 0;  // a part: the rows of the whole D and the part's first row (0, 0 otherwise)
    uint32_t* d_sets_ids = nullptr;  // hvs_assign_row_sets' id list, kept between calls
    uint32_t sets_ids_cap = 0;
    uint32_t *d_cmp_sets = nullptr, *d_sets_next = nullptr;  // per-call: hvs_compact's bounce bitmap of one set; a re-strided copy
    // the device buffers this state owns, in two lists: the per-call ones, and all (D and HvsOrdering::lp are the context's)
    template <typename... P>
    static void drop(P*&... p) { (((void)(p ? hipFree(p) : hipSuccess), p = nullptr), ...); }
    void free_call_buffers() { drop(d_cmp_bounce, d_cmp_rank, d_trim, d_cmp_sets, d_sets_next); }
    void drop_sets()
    {
        drop(d_sets);
        n_sets = sets_words = sets_part_rows = sets_row0 = 0;
    }
    void free_device()
    {
        drop(d_live, d_pad_ids, d_mask_stat, d_stale_ids, d_ilive, d_mask_ids, d_upd_rows, d_upd_ids, d_upd_from, d_sets_ids);
        drop_sets();
        free_call_buffers();
        live_cap = stale_cap = ilive_cap = mask_ids_cap = upd_cap = sets_ids_cap = 0;
    }
};

// Workspace of ONE query batch and the stream it runs on -- a "lane".  A context owns two (round 4): the last level of batch b
// ends with its re-scoring (HBM-bound gathers) and the final merge (latency-bound), both of which leave the matrix pipes idle,
// and batch b+1 begins with preparation, the exact seed and two small filter levels that cannot fill the chip; with batch
// b+1 on the other lane's stream the two ends run side by side.  hvs_ctx IS its main lane (base class: every `c->fb`,
// `c->stream` ... below means "the lane this batch runs on"); run_queries swaps the spare lane in for every other batch.
struct HvsLane {
    hipStream_t stream = nullptr;
    // sort of the batch's queries
    uint64_t *d_keys = nullptr, *d_keys_sorted = nullptr;
    uint32_t *d_qidx = nullptr, *d_qorder = nullptr;
    uint32_t *d_qra = nullptr, *d_qrb = nullptr;  // position range of each query of the batch, by batch-local index
    void* d_sort_tmp = nullptr;
    size_t sort_tmp_bytes = 0;
    uint32_t batch_cap = 0;
    // exact engine: per-(query, chunk) candidate lists
    uint64_t* d_cand = nullptr;
    uint32_t* d_cand_cnt = nullptr;
    size_t cand_lists = 0;
    // filter engines: per-slot / per-group state
    HvsBatch fb{};
    uint32_t fb_slots_cap = 0;
    size_t fb_cand_entries = 0, fb_pair_entries = 0;  // capacity of fb.cand / fb.pairs in entries
    uint32_t* d_layout = nullptr;
    // work-item lists of the current batch (HvsItems): per-quad block ranges, per-segment counts / offsets, the list
    uint32_t *d_qlo = nullptr, *d_qhi = nullptr, *d_segcnt = nullptr, *d_segoff = nullptr, *d_lvloff = nullptr, *d_cursor = nullptr;
    uint32_t* d_items = nullptr;
    size_t items_cap = 0;
    uint32_t quads_cap = 0, segs_cap = 0;
    HvsSegs segs{};  // of the current batch
    uint32_t class_counts[5] = {0, 0, 0, 0, 0};  // queries per predicate class in the current batch
};

// What a leaf of a row-partitioned context (hvs_create_partitioned) holds beside its part of D: a replica of the last
// rows of the whole D to pad from, and -- as the owner of a range of the resident queries -- the other parts' partial answers
// for that range (gather buffers, (n_parts - 1) blocks of `own` rows) and the merged answers (`own` rows), own = queries it owns
struct HvsPart {
    float* d_tail = nullptr;  // kPartTailRows x 102
    uint32_t *d_gx_ids = nullptr, *d_m_ids = nullptr;
    float *d_gx_dists = nullptr, *d_m_dists = nullptr;
    size_t gx_cap = 0, m_cap = 0;  // entries
    unsigned long long* d_padded = nullptr;
    hipEvent_t ev_x0 = nullptr, ev_x1 = nullptr, ev_m1 = nullptr;  // around the list copies and the merge kernel of the last call
    // last call
    double exchange_ms = 0.0, merge_ms = 0.0;
    uint64_t bytes = 0;
    unsigned long long padded = 0;
};
constexpr uint32_t kPartTailRows = HVS_KMAX;  // rows of the tail replica: the most a query can be padded with

// Per-query id lists and what reaches the resident queries the way they do (DESIGN 3.13a "staged attach"; 3.14, 3.17, 3.18).
// A STAGING AREA: a caller's words (CSR offsets, set indices) as they came, the four-word status block of their check kernel and
// what the host read back from it.  Nothing in force lies in one: leaf_stage fills it, the root judges every GPU's flags, and
// only then does any GPU commit.
struct HvsStage {
    uint32_t *d_words = nullptr, *d_status = nullptr;
    uint32_t cap = 0;                       // entries d_words has room for
    uint32_t flags = 0, first = 0, end = 0;  // of the words staged last: the check's flags; (offsets) offsets[0], offsets[count]
    uint32_t total() const { return flags ? 0u : end - first; }  // (the entries behind the offsets, once every pair is ascending)
    void free_device() { HvsRowSet::drop(d_words, d_status), cap = 0; }
};
// where every query's normalised list lies in an id array, and its length
struct HvsListIndex {
    uint32_t *d_begin = nullptr, *d_count = nullptr;
    uint32_t cap = 0;  // entries each of the two has room for
    void free_device() { HvsRowSet::drop(d_begin, d_count), cap = 0; }
};
// the per-query id lists of one kind in force: every query's normalised list.  While `set` is false no launch reads d_ids.
struct HvsIdLists {
    uint32_t* d_ids = nullptr;
    uint32_t ids_cap = 0;        // entries
    uint32_t nq = 0, total = 0;  // of the lists in force: the user's queries, entries of d_ids (hvs_download_*_plan)
    bool set = false, call = false;  // attached; the last call ran with them (hvs_exclude_stats, hvs_candidates_stats)
    void free_device() { HvsRowSet::drop(d_ids), ids_cap = 0, set = false; }
};

// One value of each kind per query of a set: its distance cap, normalised by hvs_k_norm_caps, and its result cursor
// -- the raw (distance, id) pair and d_after_lo = the cursor's key + 1, built from the pair by hvs_k_norm_after.
// HvsQuerySet holds two of these: the engines' and, under category sets, the user's.  Caps and cursors are sized apart
// (per_query_room): the engines' caps grow with d_q, their cursors with the first call that sets any.
struct HvsPerQuery {
    float* d_max_d2 = nullptr;
    uint64_t* d_after_lo = nullptr;
    float* d_after_dist = nullptr;
    uint32_t* d_after_id = nullptr;
    uint32_t caps_cap = 0, after_cap = 0;  // entries d_max_d2 / each of the three cursor arrays has room for
    // exclusion lists: where query q's normalised list lies in HvsQuerySet::excl.d_ids, and its length
    HvsListIndex ex;
    // shared row sets: query q's set index, or 0xFFFFFFFF for "no restriction"
    uint32_t* d_set_of = nullptr;
    uint32_t set_of_cap = 0;
    void free_device()
    {
        HvsRowSet::drop(d_max_d2, d_after_lo, d_after_dist, d_after_id, d_set_of);
        ex.free_device();
        caps_cap = after_cap = set_of_cap = 0;
    }
};

// Category sets of one GPU's resident queries (hvs_set_category_sets).  While `active`, the engines' resident set
// (hvs_ctx::d_q, nq, d_out_*, HvsQuerySet::eng) is the EXPANDED one -- `nq` sub-queries -- and this struct holds the user's
// side of it: the user's `nuq` query rows, the plan that ties a user query to its sub-queries [h_sub_off[p], h_sub_off[p + 1]),
// the user's caps and cursors (one per user query; gathered into the engines' arrays by hvs_k_expand_per_query) and the merged
// result rows.  Every resident index of the C ABI is a user index; in_* functions below translate.  Not active: nothing here is
// read, and the buffers are kept for the next attach.
struct HvsInSet {
    // The expanded set has three clients: category sets, extra query vectors, and extra clauses.  Everything
    // that ties user queries to sub-query ranges below is shared; the clients differ in staging and check, the fill and expand
    // kernels, the merge kernel and their stats.
    enum Kind { Sets, Vectors, Clauses };
    bool active = false;
    const ExpandedKind* client = nullptr;  // (while active) what the sub-queries of a user query are
    bool one_key_per_row = true;       // (while active) no row can come back under two keys: cursors may be attached
    uint32_t nuq = 0;
    std::vector<uint32_t> h_sub_off;   // nuq + 1
    std::vector<uint8_t> h_eff;        // nuq: the query is answered through its set (tests C, non-empty set)
    float* d_uq = nullptr;             // the user's rows, nuq x 104
    uint32_t *d_sub_off = nullptr, *d_set_off = nullptr, *d_parent = nullptr;  // nuq + 1, nuq + 1 (the caller's CSR offsets), nsub
    float* d_value = nullptr;          // nsub
    uint32_t uq_cap = 0, sub_cap = 0;  // user queries / sub-queries the buffers above have room for
    // extra vectors: this GPU's slice of the caller's CSR -- the offsets as they came (staged and checked before anything is
    // replaced, like HvsQuerySet::off_stage; the fill kernels read them there), and the vectors, 100 floats each
    HvsStage v_stage;
    float* d_vecs = nullptr;
    size_t vecs_cap = 0;               // floats d_vecs has room for
    // extra clauses: staged and checked in v_stage as the vectors' offsets are; their [type, v, l, r], 4 floats each,
    // and, where they bring vectors of their own, those in d_vecs
    float* d_attrs = nullptr;
    size_t attrs_cap = 0;              // floats d_attrs has room for
    HvsPerQuery user;                  // the user's caps and cursors: room for uq_cap each, allocated at attach
    uint32_t *d_m_ids = nullptr;       // merged answers, nuq x k
    float* d_m_dists = nullptr;
    size_t m_cap = 0;                  // entries
    // of the last merge: [0] under-full queries, [1] keys read, [2] (vectors, clauses) duplicates dropped, (clauses) [3] keys
    // not below the threshold, [4] chunks never loaded.  Every client's merge is given kStatWordsMin of them zeroed at least.
    static constexpr uint32_t kStatWordsMin = 3u, kStatWordsMax = 5u;
    unsigned long long* d_stat = nullptr;
    hipEvent_t ev_x0 = nullptr, ev_x1 = nullptr, ev_m0 = nullptr, ev_m1 = nullptr;  // around the expansion / the last merge
    double expand_ms = 0.0;
    // scratch of a plan made on the device (hvs_set_category_sets_device): nothing here is in force, in_commit takes from it
    uint32_t *d_p_pack = nullptr, *d_p_sub_off = nullptr;  // p_cap, p_cap + 1: the count kernel's words, the scan's offsets
    uint8_t* d_p_eff = nullptr;                            // p_cap
    unsigned long long* d_p_stat = nullptr;                // [0] flags, [1] sub-queries, [2] sub-queries if every query tested C
    uint32_t* d_p_off = nullptr;                           // a CSR on another GPU: this GPU's slice of the offsets, p_cap + 1 ...
    float* d_p_vals = nullptr;                             // ... and of the values, pv_cap; both live for that call only (in_plan_release)
    uint32_t p_cap = 0, p_off_cap = 0, pv_cap = 0;
    // last call
    bool call = false;                 // it ran on an expanded set ...
    const ExpandedKind* call_client = nullptr;  // ... of this client
    uint32_t call_set_queries = 0, call_sub = 0, call_max_set = 0;
    void free_device()
    {
        HvsRowSet::drop(d_uq, d_sub_off, d_set_off, d_parent, d_value, d_m_ids, d_m_dists, d_stat);
        HvsRowSet::drop(d_p_pack, d_p_sub_off, d_p_eff, d_p_stat, d_p_off, d_p_vals);
        HvsRowSet::drop(d_vecs, d_attrs);
        v_stage.free_device();
        p_cap = p_off_cap = pv_cap = 0;
        vecs_cap = attrs_cap = 0;
        user.free_device();
        for (hipEvent_t* ev : {&ev_x0, &ev_x1, &ev_m0, &ev_m1})
            if (*ev) (void)hipEventDestroy(*ev), *ev = nullptr;
        uq_cap = sub_cap = 0;
        m_cap = 0;
        active = false;
    }
};

// What is ATTACHED to the resident queries of one GPU: caps, cursors, category sets and the range of queries that
// have a result row.  The engines' own buffers -- d_q, nq, nq_cap, d_out_ids, d_out_dists, res_cap -- stay in hvs_ctx: every
// launch reads them and the planner probe lends them out (with the two re-run lists, which HvsCallState owns).  The invariants:
//   - while caps_set is false no launch reads eng.d_max_d2, while after_set is false none reads eng.d_after_*
//   - eng.d_max_d2 grows with d_q; the cursor arrays, once allocated, have room for eng.after_cap entries, >= nq whenever after_set
//   - while in.active, `eng` holds the EXPANDED values, one entry per sub-query, and in.user one entry per user query
//   - queries [res_lo, res_hi) have been answered with res_k slots since the set was installed (empty: none)
// It changes through the transitions below the readers and through leaf_attach.  A row-partitioned ROOT uses the same fields for
// what it keeps itself: the range of merged rows, res_gen and the two call flags.
struct HvsQuerySet {
    HvsPerQuery eng;           // what the launches read: one entry per resident query (under sets: per sub-query)
    bool caps_set = false, after_set = false;
    bool call_capped = false, call_after = false;  // the last call ran with caps / with cursors (hvs_within_stats, hvs_after_stats)
    // Exclusion lists.  excl.d_ids holds every query's normalised list (under category sets too: sub-queries read
    // their parent's through eng.ex); off_stage is where a caller's offsets are checked before anything is replaced.  While
    // excl.set is false no launch reads any of it.  While excl.set and not after_set, eng.d_after_lo holds zeros for every
    // resident query (zero_after_lo): the list forms are cursor forms.
    HvsIdLists excl;
    // Candidate lists: cand.d_ids holds every query's normalised list, cand_at where it lies.  A caller's offsets
    // are checked in off_stage too.  While cand.set is false no launch reads any of it; while it is true hvs_k_scan_candidates
    // answers every call.  Never set while in.active.
    HvsIdLists cand;
    HvsListIndex cand_at;
    HvsStage off_stage;  // the CSR offsets of exclusion and candidate lists; the normalisation kernels read them there
    // Shared row sets: the per-query set indices, in eng.d_set_of (under the expanded set: per sub-query, the
    // user's in in.user.d_set_of).  A caller's indices are checked in idx_stage before anything is replaced.
    // While rset_set is false no launch reads any of it.  While it is true the list forms of the kernels run (with_after):
    // without exclusion lists they read d_rs_zero as every query's (begin, count) -- zeros, one per resident query -- and
    // without cursors eng.d_after_lo holds zeros (zero_after_lo).
    bool rset_set = false, call_rset = false;
    HvsStage idx_stage;  // (flags: 1 = an index names no set)
    uint32_t* d_rs_zero = nullptr;
    uint32_t rs_zero_cap = 0;  // entries
    uint32_t res_lo = 0, res_hi = 0, res_k = 0;
    uint32_t set_gen = 0;      // counts the resident sets this GPU has held
    uint32_t res_gen = 0;      // set_gen of the set the range belongs to (a row-partitioned root: part 0's)
    HvsInSet in;               // the expanded set of the resident queries and its client: sets, extra vectors or extra clauses
    // every flag that says "this is attached to the resident queries", in one place: what drops, lends out or clears attachments
    // goes through it (drop_attached, DetachedForProbe, leaf_detach_flag)
    enum Attachment { kCapsOn, kCursorsOn, kExclOn, kCandOn, kRowSetsOn, kAttachments };
    bool& attached(int a) { return *std::array<bool*, kAttachments>{{&caps_set, &after_set, &excl.set, &cand.set, &rset_set}}[(size_t)a]; }
    void free_device()
    {
        eng.free_device(), in.free_device();
        excl.free_device(), cand.free_device(), cand_at.free_device(), off_stage.free_device(), idx_stage.free_device();
        HvsRowSet::drop(d_rs_zero);
        rs_zero_cap = 0;
        rset_set = false;
    }
    void drop_attached()  // caps off, cursors off, lists off, no results: they belonged to a set that is no longer the engines'
    {
        for (int a = 0; a < kAttachments; ++a) attached(a) = false;
        drop_results();
    }
    // no query has a result row: the rows (under sets the merged rows too) hold ids of a row numbering that has gone
    void drop_results() { res_lo = res_hi = 0; }
    // a call answered [q0, q0 + nq) of set `gen` with k slots: its range joins the ranges answered so far if it touches them
    void answered(uint32_t q0, uint32_t nq, uint32_t k, uint32_t gen)
    {
        if (res_gen != gen || res_k != k || res_lo >= res_hi || q0 > res_hi || q0 + nq < res_lo) {
            res_gen = gen;
            res_lo = q0;
            res_hi = q0 + nq;
            res_k = k;
        } else {
            res_lo = std::min(res_lo, q0);
            res_hi = std::max(res_hi, q0 + nq);
        }
    }
    bool covers(uint32_t nq, uint32_t k) const { return res_k == k && res_lo == 0u && res_hi >= nq; }
};

// What a call LEAVES BEHIND on one GPU until the next one: the device counters its kernels added to, the queries
// it could not answer with their re-runs, and the report that hvs_last_timing and the *_stats calls read.  The invariants:
//   - `valid`: a call has been enqueued (call_enqueued) since the last event that forgets it (call_forgotten, or a later call that
//     failed half-way).  While it is false every per-call figure reads as zero or HVS_ESTATE (call_counters, call_required);
//     hvs_last_reruns alone does not ask.
//   - `pending`: from "a call is enqueued on a filter engine" until resolve_overflow has run.  While it is true h_ovf may not have
//     arrived, pend_sn is the cut the re-runs use, and nothing reads timing.fallback_queries / retry_queries (the only copy of the
//     re-run counts) or demoted_queries.  What changes rows, index or k -- so every planner probe -- resolves first.
//   - d_ovf_list and d_retry_list hold resident query indices, with room for hvs_ctx::res_cap (ensure_results grows them with the
//     result rows); d_demote_list has room for demote_cap; d_ovf_count[0..1] are the two lists' lengths on the device.  The
//     planner probe lends d_q, d_out_* and the two lists for its own batch: the caller's survive it.
//   - d_counters (HVS_CNT_COUNT slots, hvs_device.h) are zeroed by call_begin and by the probe (counters_begin), by nothing else.
//     The filters' re-run batches add to SCANNED, RESCORED and the slots of caps and cursors (the retry pass is the call's work),
//     not to PAIRS nor to the tail and stale slots; the exact engine's re-runs send PAIRS and SCANNED to HVS_CNT_RERUN_SINK.
// It changes through call_begin, call_enqueued, call_forgotten, resolve_overflow and the launch timers.  ev_q0 / ev_q1 are also the
// stopwatch of loads, index builds and compactions.  A ROOT (multi-GPU or row-partitioned) uses host_ms and nothing else.
struct HvsCallState {
    unsigned long long* d_counters = nullptr;
    // queries without a usable bound or whose lists overflowed (-> exact engine) and queries whose guessed threshold failed its
    // check (-> a filter batch with proven thresholds), collected over all batches of a call on the device
    uint32_t *d_ovf_list = nullptr, *d_retry_list = nullptr, *d_ovf_count = nullptr;
    uint32_t* d_demote_list = nullptr;  // a call's exact list, moved aside when the tile format changes under it
    uint32_t demote_cap = 0, demoted_queries = 0;
    uint32_t* h_ovf = nullptr;  // pinned: [0] exact, [1] retry
    bool pending = false;
    uint32_t pend_sn = 0;
    hipEvent_t ev_q0 = nullptr, ev_q1 = nullptr;
    std::vector<hipEvent_t> ev_k;  // start/stop pairs around the dominant kernel's launches (grown on demand: 10^7 queries are 10 batches x 14 levels)
    int n_launch_events = 0;       // pairs used by the current call
    bool valid = false;
    hvs_timing timing{};
    double host_ms = 0.0;  // wall time of the last hvs_query (host memory in -> host memory out)
    // the queries the last call answered a second time as (device list, length), in the order their rows are fetched
    using Reruns = std::pair<const uint32_t*, uint32_t>;
    std::array<Reruns, 3> reruns() const  // exact, retry, demoted
    {
        return {{{d_ovf_list, timing.fallback_queries}, {d_retry_list, timing.retry_queries}, {d_demote_list, demoted_queries}}};
    }
};

// The host <-> device COPY PIPELINE of one GPU (who records and who waits for each event): two copy streams and three
// rings of pinned staging slots, for hvs_query's queries and result rows (PipeCall) and for uploads of rows from pageable memory
// (upload_rows).  Its fields are touched by its own functions and by PipeCall's, by nothing else.  The invariants:
//   - ev_in[i] / ev_stage are recorded on s_in, ev_out[i] on s_out, ev_batch on a COMPUTE stream (after_compute)
//   - a slot is overwritten only behind its event: h_in[i] by the host once ev_in[i] is done (stage_in), h_out_*[i] by a D2H only
//     after the host has drained it, which waits for ev_out[i] (PipeCall::drain_one)
//   - slot i has room for *_cap_q[i] queries (size_for: slots only grow) of 104 floats going in, of stage_k >= k entries coming out
//     -- the copies are strided by the current k; outd_cap_q[i] <= out_cap_q[i]: the distance slots exist only after the first call
//     that asked for distances; dma_warm is set at most once (warm_dma)
struct HvsCopyPipe {
    static constexpr uint32_t kStageQ = 65536;  // queries per staging slot
    static constexpr int kRing = 4;             // (create() and destroy() spell the ring's events out)
    hvs_ctx* owner = nullptr;  // (whose error text a failed call becomes)
    hipStream_t s_in = nullptr, s_out = nullptr;
    uint32_t in_cap_q[kRing] = {}, out_cap_q[kRing] = {}, outd_cap_q[kRing] = {};  // slot sizes in queries
    float* h_in[kRing] = {};
    uint32_t* h_out_ids[kRing] = {};
    float* h_out_dists[kRing] = {};
    hipEvent_t ev_in[kRing] = {}, ev_out[kRing] = {};
    hipEvent_t ev_batch = nullptr, ev_stage = nullptr;
    uint32_t stage_k = 0;   // k the pinned result slots were sized for
    bool dma_warm = false;  // the copy engines of s_in / s_out have moved a DMA-sized piece
    const char* create(hvs_ctx* c, hipError_t* e)  // nullptr, or the call that failed with *e
    {
        owner = c;
        for (hipStream_t* s : {&s_in, &s_out})
            if ((*e = hipStreamCreateWithFlags(s, hipStreamNonBlocking)) != hipSuccess) return "hipStreamCreate";
        for (hipEvent_t* ev : {&ev_batch, &ev_stage, &ev_in[0], &ev_out[0], &ev_in[1], &ev_out[1], &ev_in[2], &ev_out[2], &ev_in[3], &ev_out[3]})
            if ((*e = hipEventCreateWithFlags(ev, hipEventDisableTiming)) != hipSuccess) return "hipEventCreate";
        return nullptr;
    }
    void sync() const { for (hipStream_t s : {s_in, s_out}) if (s) (void)hipStreamSynchronize(s); }
    void destroy()
    {
        for (int i = 0; i < kRing; ++i)
            (void)reslot(h_in[i], in_cap_q[i], 0u, 0u), (void)reslot(h_out_ids[i], out_cap_q[i], 0u, 0u), (void)reslot(h_out_dists[i], outd_cap_q[i], 0u, 0u);
        for (hipEvent_t ev : {ev_in[0], ev_out[0], ev_in[1], ev_out[1], ev_in[2], ev_out[2], ev_in[3], ev_out[3], ev_batch, ev_stage})
            if (ev) (void)hipEventDestroy(ev);
        for (hipStream_t s : {s_in, s_out}) if (s) (void)hipStreamDestroy(s);
    }
    template <typename T>  // `slot` gets room for q queries of per_q entries each (q == 0: none), whatever it held
    int reslot(T*& slot, uint32_t& cap_q, uint32_t q, size_t per_q)
    {
        if (slot) (void)hipHostFree(slot);
        slot = nullptr, cap_q = 0u;
        if (q) HVS_HIP(owner, hipHostMalloc(reinterpret_cast<void**>(&slot), (size_t)q * per_q * sizeof(T), hipHostMallocDefault));
        cap_q = q;
        return HVS_OK;
    }
    // Slots sized by the call: nq_in queries (or as many data rows) going in and nq_out result rows of k entries coming out use
    // ceil(nq / 65536) slots of each ring, at most 4, each as large as its piece (whole slots: 27 + 26 + 26 MB, ~1 ms per 25 MB pinned)
    int size_for(uint32_t k, bool dists, uint64_t nq_in, uint64_t nq_out)
    {
        if (stage_k < k) {  // k grew (hvs_set_k): the result slots are too small
            for (int i = 0; i < kRing; ++i) (void)reslot(h_out_ids[i], out_cap_q[i], 0u, 0u), (void)reslot(h_out_dists[i], outd_cap_q[i], 0u, 0u);
            stage_k = k;
        }
        auto slot_q = [](uint64_t nq, int i) -> uint32_t {  // queries slot i has to hold (0: the call does not reach it)
            if (nq <= (uint64_t)i * kStageQ) return 0u;
            const uint64_t piece = nq > (uint64_t)kRing * kStageQ ? kStageQ : std::min<uint64_t>(kStageQ, nq - (uint64_t)i * kStageQ);
            return (uint32_t)std::min<uint64_t>(kStageQ, (piece + 4095u) / 4096u * 4096u);
        };
        for (int i = 0; i < kRing; ++i) {
            const uint32_t qi = slot_q(nq_in, i), qo = slot_q(nq_out, i);
            int rc = HVS_OK;
            if (qi > in_cap_q[i] && (rc = reslot(h_in[i], in_cap_q[i], qi, HVS_QCOLS))) return rc;
            if (qo > out_cap_q[i] && (rc = reslot(h_out_ids[i], out_cap_q[i], qo, stage_k))) return rc;
            if (dists && qo > outd_cap_q[i] && (rc = reslot(h_out_dists[i], outd_cap_q[i], qo, stage_k))) return rc;
        }
        return HVS_OK;
    }
    int stage_in(float* dst, const float* src, size_t bytes, uint32_t piece)  // piece `piece` of a transfer, pageable, through slot piece % 4
    {
        const int i = (int)(piece % (uint32_t)kRing);
        if (piece >= (uint32_t)kRing) HVS_HIP(owner, hipEventSynchronize(ev_in[i]));  // the slot's previous DMA is done
        staging_copy(h_in[i], src, bytes);
        HVS_HIP(owner, hipMemcpyAsync(dst, h_in[i], bytes, hipMemcpyHostToDevice, s_in));
        HVS_HIP(owner, hipEventRecord(ev_in[i], s_in));
        return HVS_OK;
    }
    int wait_in() { HVS_HIP(owner, hipStreamSynchronize(s_in)); return HVS_OK; }  // the host waits for s_in
    int after_compute(hipStream_t compute, hipStream_t waiter)  // `waiter` waits for what `compute` has enqueued so far
    {
        HVS_HIP(owner, hipEventRecord(ev_batch, compute));
        HVS_HIP(owner, hipStreamWaitEvent(waiter, ev_batch, 0));
        return HVS_OK;
    }
    // The first operation on a stream creates its hardware queue (and the first copy in each direction its DMA path): a few ms that
    // belong to hvs_create, not inside the first query (round 3's cold hvs_query of 10^4 queries took 8 ms for 2 ms of device work)
    void warm_streams(hipStream_t lane0, hipStream_t lane1, uint32_t* d_two, uint32_t* h_two)
    {
        for (hipStream_t lane : {lane0, lane1}) {
            (void)hipMemsetAsync(d_two, 0, 2 * sizeof(uint32_t), lane);
            (void)hipStreamSynchronize(lane);
        }
        (void)hipMemcpyAsync(d_two, h_two, 2 * sizeof(uint32_t), hipMemcpyHostToDevice, s_in);
        (void)hipStreamSynchronize(s_in);
        (void)hipMemcpyAsync(h_two, d_two, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s_out);
        (void)after_compute(lane0, s_out);
        (void)hipStreamSynchronize(s_out);
        (void)hipGetLastError();
    }
    // The first DMA-sized copy in each direction sets up its engine queue (a cold 4 MB D2H took 6 ms): in hvs_reserve, not in the first query
    void warm_dma(uint32_t* d_ids, float* d_q, size_t call_bytes)
    {
        const size_t bytes = std::min<size_t>((size_t)1 << 20, std::min((size_t)out_cap_q[0] * stage_k * sizeof(uint32_t),
                                                                      (size_t)in_cap_q[0] * HVS_QCOLS * sizeof(float)));
        if (dma_warm || !h_out_ids[0] || !h_in[0] || !d_ids || !d_q || !bytes || call_bytes < bytes) return;
        (void)hipMemcpyAsync(h_out_ids[0], d_ids, bytes, hipMemcpyDeviceToHost, s_out);
        (void)hipMemcpyAsync(d_q, h_in[0], bytes, hipMemcpyHostToDevice, s_in);
        (void)hipStreamSynchronize(s_out);
        (void)hipStreamSynchronize(s_in);
        (void)hipGetLastError();
        dma_warm = true;
    }
};

// What ONE batch of a call on two lanes waits for between its preparation and its seed, and records behind the filter launches of
// its level before the last and of its last level.  All null (the default: retry batches, the planner probe): nothing of either.
struct BatchGates { hipEvent_t wait_heavy = nullptr, record_pdone = nullptr, record_fdone = nullptr; };

// The HAND-OVER between the two lanes of a call (HvsLane).  Slot b & 1 of the two event pairs belongs to batch b.
//   - ev_fdone: end of the LAST level's filter launch of the lane's latest batch.  The next batch (other lane) runs its seed behind
//     it -- its head then runs beside this batch's last re-scoring and final merge, not beside its filter launches (two crews of
//     filter workgroups streaming different tiles through the same L2s: measured 12 % slower than one lane).
//   - ev_pdone: likewise the end of the filter launch of the level BEFORE the last.  The next batch's preparation (query sort, slot
//     layout, fragments, work-item lists -- memory- and latency-bound) starts behind it and runs beside this batch's re-scoring of
//     that level; its compute-heavy part (exact seed, low filter levels) waits for ev_fdone (BatchGates::wait_heavy).
//   - ev_lane: end of the spare lane's latest batch.  lanes_failed: no room for a second workspace (ensure_spare_lane); never cleared.
struct HvsLaneGates {
    bool lanes_failed = false;
    hipEvent_t ev_lane = nullptr;
    hipEvent_t ev_fdone[2] = {nullptr, nullptr}, ev_pdone[2] = {nullptr, nullptr};
    hipError_t create()
    {
        hipError_t e = hipSuccess;
        for (hipEvent_t* ev : {&ev_lane, &ev_fdone[0], &ev_fdone[1], &ev_pdone[0], &ev_pdone[1]})
            if ((e = hipEventCreateWithFlags(ev, hipEventDisableTiming)) != hipSuccess) break;
        return e;
    }
    void destroy() { for (hipEvent_t ev : {ev_lane, ev_fdone[0], ev_fdone[1], ev_pdone[0], ev_pdone[1]}) if (ev) (void)hipEventDestroy(ev); }
    // batch b > 0 of a call on two lanes over K >= 1 filter levels: what its stream waits for before anything of it is enqueued
    hipEvent_t start_of(size_t b, uint32_t K) const { return K >= 2u ? ev_pdone[(b - 1u) & 1u] : ev_fdone[(b - 1u) & 1u]; }
    BatchGates of_batch(size_t b, bool have_prev) const { return {have_prev ? ev_fdone[(b - 1u) & 1u] : nullptr, ev_pdone[b & 1u], ev_fdone[b & 1u]}; }
};

struct hvs_ctx : HvsLane {
    int device = 0;
    HvsLane spare;       // the second lane (its buffers are allocated by the first call that has two batches)
    HvsLaneGates gates;  // the two lanes' hand-over events
    int engine = HVS_ENGINE_AUTO;
    bool scalar_order = false;  // baseline engine's summation order (exact engine only)
    uint32_t k = HVS_KNN;       // neighbours per query (hvs_set_k; the reference's KNN_LIMIT, optimized_impl.h:26)
    int cap = 256;              // candidate-list capacity the kernels run with: 256 (k <= 128) or 512 (k <= 256)
    bool padding = true;        // pad answers with the last rows of D (off: partial answers of a data shard)
    std::string err;

    // data set, raw rows n x 102 (the io.h layout) resident in HBM; which of the n rows are live, stale or behind the index: `rs`
    float* d_data = nullptr;
    uint32_t n = 0;
    double load_ms = 0.0;
    HvsRowSet rs;

    // resident queries + results; what is attached to them -- caps, cursors, category sets, the answered range: `qs`
    float* d_q = nullptr;
    uint32_t nq = 0, nq_cap = 0;
    uint32_t* d_out_ids = nullptr;
    float* d_out_dists = nullptr;
    uint32_t res_cap = 0;
    HvsQuerySet qs;
    HvsCallState call;  // what the last call left behind: counters, re-run lists, the report

    // ---- MFMA engine: index over D (two orderings) ...
    // Two facts: `have_order` -- keys and perm of both orderings exist (the exact engine's range scans need no more) -- and
    // `fmt.built != HVS_FMT_NONE` -- usable tiles exist on top of them.  Tiles imply orderings; free_index drops both.
    // A third, beside them: `n_indexed` -- the rows both orderings (and the tiles) cover, = n at every index build and 0
    // without orderings.  Everything built over POSITIONS (perm, bpos, tiles, lp, the level table) is sized by it.
    bool have_order = false;
    uint32_t n_indexed = 0;
    HvsFormatState fmt;
    HvsLevels lv{};                       // same block count for both orderings
    HvsOrdering ord[2];  // [0] the (C,T) ordering, [1] the T ordering
    HvsBounds* d_bounds = nullptr;
    HvsQuant* d_quant = nullptr;                          // INT8 format: centre and scale
    double index_ms = 0.0;
    bool index_too_large = false;  // more than 2^27 rows: no filter index (hvs_timing.flags says so)
    // (the per-batch state of the filter engines lives in the lanes)
    int num_cus = 256;
    HvsGuessTable guess_tab[13]{};  // order statistics of the guessed thresholds for k = guess_k: [0] proven (retry batches),
    bool guess_have[13] = {};       // [p] failure target 10^-p
    uint32_t guess_k = 0;

    HvsCopyPipe pipe;         // host <-> device pipeline of hvs_query and of uploads: copy streams + rings of pinned staging slots
    uint32_t reserve_nq = 0;  // hvs_reserve: queries per call the caller announced
    // planner probe (probe_format): the probe batch of 1024 queries stands for the large batches the format will serve, so it
    // runs with THEIR failure target -- and with their list capacity (HVS_FCAP entries per query and level): a format whose band
    // overflows that capacity fails in production too
    uint32_t force_pfail = 0;

    // multi-GPU root (hvs_create_multi): owns one leaf context per GPU; D is replicated, the queries of a call are cut
    // into one contiguous range per leaf (optimized_parallel.hpp:91: iterations are independent) and every leaf
    // writes its block of ids straight into its slice of the caller's buffer
    void* trace = nullptr;  // HVS_TRACE: the HostTrace of the running hvs_load_data
    std::vector<int> node_cpus;  // CPUs of the NUMA node this GPU hangs off (empty: unknown); the leaf's host thread runs there
    std::vector<hvs_ctx*> kids;
    std::vector<uint32_t> kid_q0;  // resident queries: first global index of each leaf's range (kids.size() + 1 entries)
    int gather_mode = 0;           // HVS_GATHER_DIRECT / HVS_GATHER_PEER

    // row-partitioned root (hvs_create_partitioned): leaf r holds global rows [part_row0[r], part_row0[r + 1]) as ITS rows 0..,
    // with padding off; every leaf holds all resident queries and kid_q0 cuts them into owner ranges
    bool partitioned = false;
    uint32_t part_n = 0;               // rows of the whole D (0: no data set loaded)
    std::vector<uint32_t> part_row0;   // kids.size() + 1 entries
    hvs_partition_info pinfo{};
    bool part_timing_valid = false;
    uint32_t part_call_nq = 0;         // queries of the last call
    HvsPart part;                      // (of a leaf of such a root)
};

namespace {

// ---- readers of the row-set state (HvsRowSet).  The two roles of the mask.  `masked`: some row is dead or some
// index entry is stale -- the MASKED kernels run, pairs are counted the masked way, no host-side range counts.  Launches that
// reach a row by its id in D take rs.d_live; launches that reach it through the index (perm, tiles) take index_mask(c).
bool masked(const hvs_ctx* c) { return c->rs.n_dead != 0u || !c->rs.h_stale.empty(); }
// the resident queries carry distance caps: the CAPPED kernels run (with_capped)
bool capped(const hvs_ctx* c) { return c->qs.caps_set; }
// ... carry result cursors: the AFTER kernels run (with_capped_after)
bool has_after(const hvs_ctx* c) { return c->qs.after_set; }
// ... carry exclusion lists: the EXCL forms of the AFTER kernels run (with_after)
bool has_excl(const hvs_ctx* c) { return c->qs.excl.set; }
// ... carry set indices of shared row sets: the same forms run, with the set's bit as one more admission test
bool has_rset(const hvs_ctx* c) { return c->qs.rset_set && c->rs.n_sets != 0u; }
// what the list forms receive: the lists (or, while only set indices are attached, empty lists for every query: d_rs_zero) and
// the sets (or none: set_of == nullptr)
HvsExcl excl_arg(const hvs_ctx* c)
{
    const HvsQuerySet& s = c->qs;
    HvsExcl x{s.eng.ex.d_begin, s.eng.ex.d_count, s.excl.d_ids, nullptr, nullptr, 0u, 0u};
    if (!s.excl.set) x.begin = x.count = x.ids = s.d_rs_zero;
    if (has_rset(c)) {
        x.set_of = s.eng.d_set_of;
        x.set_bits = c->rs.d_sets;
        x.set_words = c->rs.sets_words;
        x.row0 = c->rs.sets_row0;
    }
    return x;
}
// ... carry candidate lists: hvs_k_scan_candidates answers, whatever engine is selected (run_candidates)
bool has_cand(const hvs_ctx* c) { return c->qs.cand.set; }
// the resident set as the caller sees it (HvsInSet): under an expanded set the user's queries and the merged rows
uint32_t user_nq(const hvs_ctx* c) { return c->qs.in.active ? c->qs.in.nuq : c->nq; }
const float* user_queries(const hvs_ctx* c) { return c->qs.in.active ? c->qs.in.d_uq : c->d_q; }
const uint32_t* user_ids(const hvs_ctx* c) { return c->qs.in.active ? c->qs.in.d_m_ids : c->d_out_ids; }
const float* user_dists(const hvs_ctx* c) { return c->qs.in.active ? c->qs.in.d_m_dists : c->d_out_dists; }
// every resident query has a result row with the current k (hvs_set_after_from_results needs all of them)
bool leaf_has_all_results(const hvs_ctx* c) { return c->qs.covers(c->nq, c->k); }

// ---- HvsCallState's smallest transition (DESIGN 3.5a has the table; the others follow the launch timers).  Nothing of the last
// call is left to report until the next one (hvs_last_timing: HVS_ESTATE; the per-call figures of hvs_mask_stats,
// hvs_append_stats and hvs_update_stats: zero): category sets, a new k or a compaction re-sized or renumbered what it answered;
// the planner probe ran its own batch through the call counters and the launch timers, and the probe's figures must not be
// reported under the caller's last query's name; a multi-GPU call gave this GPU no queries, or no row of the sampled prefix.
int call_forgotten(hvs_ctx* c)
{
    c->call.valid = false;
    c->call.n_launch_events = 0;  // (the launch timers are free again)
    return HVS_OK;
}

// ---- transitions of the resident-query state (HvsQuerySet; DESIGN 3.13a has the table) ----
// a call replaces the resident set: sets, caps and cursors belonged to the old one, and so did its results
void resident_set_replaced(hvs_ctx* c)
{
    c->qs.in.active = false;
    c->qs.drop_attached();
    ++c->qs.set_gen;
}
// the expanded set's client -- category sets, extra vectors or extra clauses -- attached (`on`), detached, or lost half-way
// through an attach: the engines' set changed under everything else that was attached -- caps, cursors and lists come after
// the client, earlier results are dropped, the last call's figures with them
void expanded_changed(hvs_ctx* c, bool on)
{
    c->qs.in.active = on;
    c->qs.drop_attached();
    call_forgotten(c);
}
// k changed: no result row and no merged row has the new size (the range itself is told by res_k), nothing of the last call is
// left to report.  Returns the queries the result buffers had room for: hvs_set_k re-sizes them at once.
uint32_t k_changed(hvs_ctx* c)
{
    const uint32_t had = c->res_cap;
    c->res_cap = 0;
    c->qs.in.m_cap = 0;  // (the merged rows of the expanded set, whichever client's, are re-allocated by the next call)
    call_forgotten(c);
    return had;
}
// the planner probe runs its own queries through the context: caps and cursors belong to the caller's, and wait outside
struct DetachedForProbe {
    HvsQuerySet& s;
    bool was[HvsQuerySet::kAttachments];
    explicit DetachedForProbe(HvsQuerySet& qs) : s(qs)
    {
        for (int a = 0; a < HvsQuerySet::kAttachments; ++a) was[a] = s.attached(a), s.attached(a) = false;
    }
    ~DetachedForProbe()
    {
        for (int a = 0; a < HvsQuerySet::kAttachments; ++a) s.attached(a) = was[a];
    }
};
const uint32_t* index_mask(const hvs_ctx* c) { return c->rs.h_stale.empty() ? c->rs.d_live : c->rs.d_ilive; }
uint32_t tail_rows(const hvs_ctx* c) { return c->have_order ? c->n - c->n_indexed : 0u; }
uint32_t stale_below(const hvs_ctx* c, uint32_t sn)
{
    if (!c->have_order || c->rs.h_stale.empty()) return 0u;
    return (uint32_t)(std::lower_bound(c->rs.h_stale.begin(), c->rs.h_stale.end(), sn) - c->rs.h_stale.begin());
}
// rows behind the index, stale rows aside: the tail -- or, without orderings, the rows that came after the last attempt to build one
uint32_t rows_behind_index(const hvs_ctx* c) { return c->have_order ? c->n - c->n_indexed : c->n - std::min(c->n, c->rs.index_tried_n); }
// rows_behind_index + n_stale above which an append or an update re-indexes before it returns (fold_if_over_limit).  Default
// max(4096, n_indexed >> 10), derived, then measured at a loss of 15 % at the limit: if the tail scan evaluated pairs at the exact engine's rate, ~3.1 x 10^11
// pairs/s on record, and the filter engines answer a flagship query in ~310 ns, 10^4 tail rows (n_indexed = 10^7) cost a tenth of a query.
uint32_t tail_limit_of(const hvs_ctx* c) { return c->rs.tail_limit ? c->rs.tail_limit : std::max(4096u, c->n_indexed >> 10); }

// ---- mask words: ceil(n / 64) u64 words, row i at bit i & 63 of word i >> 6 (the device reads the same bytes as u32 words)
inline size_t mask_words(uint32_t n) { return ((size_t)n + 63u) / 64u; }
// word w with the bits past n cleared (bits == nullptr: every row live)
inline uint64_t masked_word(const uint64_t* bits, uint32_t n, size_t w)
{
    const uint64_t v = bits ? bits[w] : ~0ull;
    return w + 1u == mask_words(n) && (n & 63u) ? v & ((1ull << (n & 63u)) - 1ull) : v;
}
inline uint32_t mask_popcount(const uint64_t* bits, uint32_t n)  // live rows among the n
{
    const size_t W = mask_words(n);
    uint32_t live = 0;  // (whole words in a plain loop: every delete walks the whole mask, 1.6 x 10^5 words at 10^7 rows)
    for (size_t w = 0; w + 1u < W; ++w) live += (uint32_t)__builtin_popcountll(bits[w]);
    return W ? live + (uint32_t)__builtin_popcountll(masked_word(bits, n, W - 1u)) : live;
}
inline uint32_t mask_half(uint64_t word, size_t i) { return (uint32_t)(word >> (32u * (i & 1u))); }  // u32 word i of the device's view
inline void mask_set_range(std::vector<uint64_t>& bits, uint32_t a, uint32_t b)  // rows [a, b) live
{
    for (uint32_t i = a; i < b;) {
        const uint32_t at = i & 63u, m = std::min(64u - at, b - i);
        bits[i >> 6] |= (m == 64u ? ~0ull : ((1ull << m) - 1ull)) << at;
        i += m;
    }
}

uint32_t env_u32(const char* name, uint32_t dflt, uint32_t lo, uint32_t hi)
{
    const char* v = std::getenv(name);
    if (!v || !*v) return dflt;
    const unsigned long x = std::strtoul(v, nullptr, 10);
    return x < lo ? lo : (x > hi ? hi : (uint32_t)x);
}
// queries answered per pass over D; HVS_EXACT_BATCH / HVS_MFMA_BATCH override (tests use small batches)
const uint32_t kBatch = env_u32("HVS_EXACT_BATCH", 65536u, 64u, 1u << 20);
const uint32_t kBatchMfma = env_u32("HVS_MFMA_BATCH", 1u << 21, 128u, 1u << 21);  // (2^21: +2.2 % queries/s over 2^20, 34 GB of batch state)
// re-scoring blocks per group (each stages the group's 128 queries in LDS): HVS_RESCORE_BLOCKS overrides
const uint32_t kRescoreBlocks = env_u32("HVS_RESCORE_BLOCKS", 0u, 0u, 64u);  // 0: chosen per batch
// small batches: level 0 (the exact seed kernel) is cut into chunks until about this many waves are in flight
const uint32_t kSeedWaves = env_u32("HVS_SEED_WAVES", 16384u, 64u, 1u << 20);
// INT8 tiles are built for v_mfma_i32_16x16x64_i8 (HVS_FMT_I8X16: 1.16x the pair rate of the 32x32x32 shape in the
// filter loop, scripts/mfma_shape_lab.hip); HVS_I8_SHAPE=32 selects the 32x32x32 layout (HVS_FMT_I8) for A/B runs
const int kI8Fmt = env_u32("HVS_I8_SHAPE", 16u, 16u, 32u) == 32u ? HVS_FMT_I8 : HVS_FMT_I8X16;
// Level radices of the index (powers of two; see "Guessed thresholds" at hvs_k_merge)
uint32_t pow2_floor(uint32_t x) { uint32_t p = 2u; while (p * 2u <= x) p *= 2u; return p; }
const uint32_t kRadixLast = pow2_floor(env_u32("HVS_RADIX_LAST", HVS_RADIX_LAST, 2u, 64u));
const uint32_t kRadixMid = pow2_floor(env_u32("HVS_RADIX_MID", HVS_RADIX_MID, 2u, 64u));
// HVS_RADICES="4,8,32": the radices of the last levels, last level first (A/B runs); HVS_RADIX_MID continues behind them
struct RadixPlan {
    uint32_t r[16] = {};
    bool set = false;
    RadixPlan()
    {
        const char* v = std::getenv("HVS_RADICES");
        if (!v || !*v) return;
        int k = 0;
        bool ok = true;
        while (*v && k < 14) {
            char* end = nullptr;
            const unsigned long x = std::strtoul(v, &end, 10);
            if (end == v) {  // not a number ("4;8", "4x"): the whole variable is ignored
                ok = false;
                break;
            }
            v = end;
            if (x >= 2 && x <= 64) r[k++] = pow2_floor((uint32_t)x);
            while (*v == ',' || *v == ' ') ++v;
        }
        if (!ok) {
            for (uint32_t& x : r) x = 0u;
            k = 0;
        }
        set = k > 0;
    }
};
const RadixPlan kRadixPlan;
// smallest order statistic a guessed threshold may use, and -log10 of the chance that one guess leaves fewer than k rows
// below it (plan_guess)
const uint32_t kGuessMid = env_u32("HVS_GUESS_MID", 3u, 1u, 256u);
// HVS_GUESS_PFAIL unset (0): by batch size -- 10^-3 for batches of 2^18 queries and more, 10^-4 from 2^15, 10^-5 below: a
// retry batch costs a fixed ~0.8 ms of latency-bound rounds whatever its size, which a batch of 10^4 queries (2.6 ms)
// cannot afford every time while a batch of 2^21 (650 ms) gains 3 % from the tighter guesses
const uint32_t kGuessPfail = env_u32("HVS_GUESS_PFAIL", 0u, 0u, 12u);
// (round 4: 10^-6 below 2^15 queries -- measured on BASELINE configs[1]/[2], 10^4 queries per batch: a failed guess costs the call a
// host synchronisation and a retry batch of ~0.55 ms whose kernels are launch-bound; 10^-5 retried 0.3-0.45 queries per call,
// 10^-6 none in 20 calls for 11 % more candidates: 2.21 / 1.80 ms per call against 2.27 / 1.90, profiles/r04/configs12_sweeps.txt)
uint32_t guess_pfail_for(uint32_t nqb) { return kGuessPfail ? kGuessPfail : (nqb >= (1u << 18) ? 3u : (nqb >= (1u << 15) ? 4u : 6u)); }
constexpr uint32_t kMfmaMinRows = 32768;  // below this the exact engine is used by HVS_ENGINE_AUTO
constexpr uint32_t kIndexMinRows = 4096;  // below this no index is built (the exact engine scans all rows)

// two lanes (see HvsLane): HVS_LANES=0 keeps every batch on the main lane (A/B runs)
const bool kLanes = env_u32("HVS_LANES", 1u, 0u, 1u) != 0u;
void swap_lanes(hvs_ctx* c) { std::swap(static_cast<HvsLane&>(*c), c->spare); }
struct LaneGuard {  // the spare lane is swapped in for the duration of one batch, whatever way the batch ends
    hvs_ctx* c;
    bool on;
    ~LaneGuard()
    {
        if (on) swap_lanes(c);
    }
};
void free_lane(HvsLane& L)
{
    HvsBatch& B = L.fb;
    void* ptrs[] = {L.d_keys, L.d_keys_sorted, L.d_qidx, L.d_qorder, L.d_qra, L.d_qrb, L.d_sort_tmp, L.d_cand, L.d_cand_cnt,
                    B.qid, B.rank, B.ra, B.rb, B.gua, B.gub, B.gord, B.bfrag, B.theta, B.qn, B.normq, B.eq, B.nqb,
                    B.top, B.topcnt, B.tau, B.cand, B.candcnt, B.overflow, B.pairs, B.paircnt, B.goverflow,
                    L.d_layout, L.d_qlo, L.d_qhi, L.d_segcnt, L.d_segoff, L.d_lvloff, L.d_cursor, L.d_items};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (L.stream) (void)hipStreamDestroy(L.stream);
    L = HvsLane{};
}

// HVS_TRACE=1: hvs_query prints the host-side phases of a call (microseconds since its start) to stderr -- where a small
// call's wall time goes between the caller's buffers and the first / last kernel
const bool kTrace = env_u32("HVS_TRACE", 0u, 0u, 1u) != 0u;
struct HostTrace {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    std::string line;
    void mark(const char* what)
    {
        if (!kTrace) return;
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        char buf[96];
        std::snprintf(buf, sizeof(buf), " %s@%.0f", what, us);
        line += buf;
    }
    void flush(const char* tag, uint32_t nq)
    {
        if (kTrace) std::fprintf(stderr, "[hvs trace] %s nq=%u:%s\n", tag, nq, line.c_str());
    }
};

void trace_mark(hvs_ctx* c, const char* what)
{
    if (kTrace && c->trace) static_cast<HostTrace*>(c->trace)->mark(what);
}

int fail(hvs_ctx* c, int code, const std::string& msg)
{
    if (c) c->err = msg;
    return code;
}

template <typename T>
int dev_alloc(hvs_ctx* c, T** p, size_t count)
{
    if (*p) {
        (void)hipFree(*p);
        *p = nullptr;
    }
    if (count == 0) return HVS_OK;
    HVS_HIP(c, hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T)));
    return HVS_OK;
}

// Room for n entries in *p -- and in every one of `more`, buffers that grow together under the one capacity -- whatever they
// held: contents are NOT kept (grow_keep keeps them), a failure leaves the capacity at 0, and nothing happens while n fits.
template <typename Cap, typename T, typename... More>
int ensure_room(hvs_ctx* c, T** p, Cap& cap, size_t n, More**... more)
{
    if (n <= cap) return HVS_OK;
    cap = 0;
    int rc = dev_alloc(c, p, n);
    ((rc = rc ? rc : dev_alloc(c, more, n)), ...);
    if (!rc) cap = (Cap)n;
    return rc;
}

// room for n caps and / or n cursors in `v`
enum : unsigned { kCaps = 1u, kCursors = 2u };
int per_query_room(hvs_ctx* c, HvsPerQuery& v, unsigned which, uint32_t n)
{
    int rc = which & kCaps ? ensure_room(c, &v.d_max_d2, v.caps_cap, n) : HVS_OK;
    if (!rc && (which & kCursors)) rc = ensure_room(c, &v.d_after_lo, v.after_cap, n, &v.d_after_dist, &v.d_after_id);
    return rc;
}

// Device temporaries of one scope, freed when it ends, whichever way it ends.  `lend`: the temporary also stands in for one of
// the context's long-lived buffers for that time (swapped into `*field` now, swapped back before it is freed).
struct ScopedDevBufs {
    void* buf[5] = {};
    void** lent[5] = {};
    int count = 0;
    ScopedDevBufs() = default;
    ScopedDevBufs(const ScopedDevBufs&) = delete;
    ScopedDevBufs& operator=(const ScopedDevBufs&) = delete;
    template <typename T>
    hipError_t alloc(T** out, size_t n)
    {
        if (count == 5) return hipErrorInvalidValue;
        const hipError_t e = hipMalloc(&buf[count], n * sizeof(T));
        if (e != hipSuccess) return e;
        *out = static_cast<T*>(buf[count++]);
        return hipSuccess;
    }
    template <typename T>
    hipError_t lend(T** field, size_t n)
    {
        T* mine = nullptr;
        const hipError_t e = alloc(&mine, n);
        if (e != hipSuccess) return e;
        lent[count - 1] = reinterpret_cast<void**>(field);
        std::swap(*lent[count - 1], buf[count - 1]);
        return hipSuccess;
    }
    ~ScopedDevBufs()
    {
        while (count-- > 0) {
            if (lent[count]) std::swap(*lent[count], buf[count]);
            if (buf[count]) (void)hipFree(buf[count]);
        }
    }
};

// Event pair around one launch of the dominant kernel (HIP events on the library's own stream: bench.py's roofline
// reads their sum).  begin returns the pair's index or -1 (events could not be created: the launch goes untimed).
int kernel_timer_begin(hvs_ctx* c)
{
    HvsCallState& s = c->call;
    const int ev = s.n_launch_events;
    while (s.ev_k.size() < 2u * (size_t)(ev + 1)) {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return s.timing.untimed_launches++, -1;
        s.ev_k.push_back(e);
    }
    if (hipEventRecord(s.ev_k[2 * ev], c->stream) != hipSuccess) return s.timing.untimed_launches++, -1;
    return ev;
}
void kernel_timer_end(hvs_ctx* c, int ev)
{
    if (ev < 0) return;
    if (hipEventRecord(c->call.ev_k[2 * ev + 1], c->stream) == hipSuccess)
        c->call.n_launch_events = ev + 1;
    else
        c->call.timing.untimed_launches++;  // (main_kernel_ms is then a lower bound: bench.py refuses to price a roofline from it)
}

// ---- transitions and readers of the call state (HvsCallState; DESIGN 3.5a has the table) ----
// the counters start a batch's worth of counting at zero: a call's, or the planner probe's own batch
int counters_begin(hvs_ctx* c)
{
    HVS_HIP(c, hipMemsetAsync(c->call.d_counters, 0, HVS_CNT_COUNT * sizeof(unsigned long long), c->stream));
    HVS_HIP(c, hipMemsetAsync(c->call.d_ovf_count, 0, 2 * sizeof(uint32_t), c->stream));
    return HVS_OK;
}
// A call begins (the one before it is resolved): no report until it is enqueued, no launch timed, no re-run counted (a list of
// an earlier call must never be scattered into this call's results), the counters at zero; ev_q0 opens its device time.
int call_begin(hvs_ctx* c)
{
    HvsCallState& s = c->call;
    s.valid = false;
    s.n_launch_events = 0;
    s.timing = hvs_timing{};
    s.demoted_queries = 0;
    if (int rc = counters_begin(c)) return rc;
    HVS_HIP(c, hipEventRecord(s.ev_q0, c->stream));
    return HVS_OK;
}
// hvs_timing.engine of a call that the tiles of format `fmt` filtered
int timing_engine_for(int fmt) { return HVS_IS_I8(fmt) ? HVS_ENGINE_MFMA_I8 : fmt == HVS_FMT_F16 ? HVS_ENGINE_MFMA_F16 : HVS_ENGINE_MFMA_FILTER; }
// The call's `nq` queries are enqueued: ev_q1 closes its device time (resolve_overflow moves it behind the re-runs), a filter
// engine's fail counts are on their way to h_ovf (`filtered`; `sn`: the cut its re-runs will use), there is a call to report.
int call_enqueued(hvs_ctx* c, uint32_t nq, bool filtered, uint32_t sn)
{
    HvsCallState& s = c->call;
    HVS_HIP(c, hipEventRecord(s.ev_q1, c->stream));
    if (filtered) {
        HVS_HIP(c, hipMemcpyAsync(s.h_ovf, s.d_ovf_count, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        s.pending = true;
        s.pend_sn = sn;
    }
    s.timing.nq = nq;
    s.timing.engine = filtered ? timing_engine_for(c->fmt.built) : HVS_ENGINE_EXACT_SCAN;
    s.timing.load_ms = c->load_ms;
    s.timing.n_gpus = 1;
    s.timing.flags = (c->index_too_large ? HVS_TIMING_INDEX_TOO_LARGE : 0u) | (filtered && HVS_IS_I8(c->fmt.built) && c->fmt.built_rot ? HVS_TIMING_I8_ROTATED : 0u);
    s.valid = true;
    return HVS_OK;
}
// the exact list's length (and the retry list's) as the device has it now, through h_ovf -- nothing is pending; waits for the stream
int fetch_fail_counts(hvs_ctx* c, uint32_t* exact, uint32_t* retry = nullptr)
{
    HVS_HIP(c, hipMemcpyAsync(c->call.h_ovf, c->call.d_ovf_count, (retry ? 2 : 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    *exact = c->call.h_ovf[0];
    if (retry) *retry = c->call.h_ovf[1];
    return HVS_OK;
}
// where an exact-engine batch adds its PAIRS and SCANNED: the call's counters, or the sink (re-runs; sub-batches counted beforehand)
unsigned long long* exact_batch_counters(hvs_ctx* c, bool counted) { return c->call.d_counters + (counted ? 0 : HVS_CNT_RERUN_SINK); }
// how hvs_last_timing, hvs_within_stats, hvs_after_stats and hvs_in_stats begin: there is a last call to report (else HVS_ESTATE),
// and it is resolved and complete
int leaf_sync(hvs_ctx* c);
int call_required(hvs_ctx* c) { return c->call.valid ? leaf_sync(c) : fail(c, HVS_ESTATE, "no query has run yet"); }
// The one reader of the counters: slots [first, first + N) of the last call, or zeros when there is none to report (as
// hvs_mask_stats, hvs_append_stats and hvs_update_stats say it).  `own_batch`: the planner probe reads its own batch's.
template <size_t N>
int call_counters(hvs_ctx* c, int first, unsigned long long (&v)[N], bool own_batch = false)
{
    std::fill(v, v + N, 0ull);
    if (c->call.valid || own_batch) HVS_HIP(c, hipMemcpy(v, c->call.d_counters + first, sizeof(v), hipMemcpyDeviceToHost));
    return HVS_OK;
}

// the select / merge / scan kernels exist for two list capacities; `f` gets the capacity as a compile-time constant
template <typename F>
void with_cap(int cap, F f)
{
    if (cap == 512)
        f(std::integral_constant<int, 512>{});
    else
        f(std::integral_constant<int, 256>{});
}

// ... and for the two forms of the kernels that read the live-row mask: `f` gets (capacity, masked) as compile-time constants;
// masked only while at least one row is dead or stale
template <typename F>
void with_cap_mask(const hvs_ctx* c, F f)
{
    with_cap(c->cap, [&](auto CAPT) {
        if (masked(c))
            f(CAPT, std::true_type{});
        else
            f(CAPT, std::false_type{});
    });
}

// ... and for the exact engine's kernels, which also exist for the two summation orders: `f` gets (scalar order, capacity,
// masked)
template <typename F>
void with_order_cap_mask(const hvs_ctx* c, F f)
{
    with_cap_mask(c, [&](auto CAPT, auto MT) {
        if (c->scalar_order)
            f(std::true_type{}, CAPT, MT);
        else
            f(std::false_type{}, CAPT, MT);
    });
}

// ... and for the kernels that have a capped form: `f` gets "capped" as one more compile-time constant, true only
// while the resident queries carry caps
template <typename F>
void with_capped(const hvs_ctx* c, F f)
{
    if (capped(c))
        f(std::true_type{});
    else
        f(std::false_type{});
}

// ... and for the kernels that also have a cursor form: `f` gets (capped, after); after only while the resident
// queries carry cursors
// ... and, on the cursor forms only, a list form: `f` gets (after, excl) with excl only while the resident queries
// carry exclusion lists; lists without cursors run the cursor form with an after_lo of zeros (zero_after_lo), which admits
// every key, so the plain and the cursor forms are launched exactly as they were while no lists are set
template <typename F>
void with_after(const hvs_ctx* c, F f)
{
    if (has_excl(c) || has_rset(c))  // (set indices of shared row sets ride in the list forms: DESIGN 3.18)
        f(std::true_type{}, std::true_type{});
    else if (has_after(c))
        f(std::true_type{}, std::false_type{});
    else
        f(std::false_type{}, std::false_type{});
}
template <typename F>
void with_capped_after(const hvs_ctx* c, F f)
{
    with_capped(c, [&](auto WT) { with_after(c, [&](auto AT, auto XT) { f(WT, AT, XT); }); });
}

// the k best of every query's candidate lists to the output rows (hvs_k_select): `nsel` queries named by `qlist`, each with
// `nchunks` lists of which list 0 of the first query is `cand` / `cnt` and consecutive queries' lists lie `stride` apart
void launch_select(hvs_ctx* c, const uint32_t* qlist, uint32_t nsel, uint32_t stride, uint32_t nchunks, uint64_t* cand, uint32_t* cnt)
{
    with_order_cap_mask(c, [&](auto ST, auto CAPT, auto MT) {
        with_capped_after(c, [&](auto WT, auto AT, auto XT) {
            hipLaunchKernelGGL((hvs_k_select<decltype(ST)::value, decltype(CAPT)::value, decltype(MT)::value, decltype(WT)::value, decltype(AT)::value, decltype(XT)::value>),
                               dim3((nsel + 3u) / 4u), dim3(256), 0, c->stream, c->d_data, c->n, c->d_q, qlist, nsel, stride, nchunks, cand, cnt,
                               c->padding ? 1 : 0, c->d_out_ids, c->d_out_dists, c->k, c->rs.d_pad_ids, c->qs.eng.d_max_d2, c->call.d_counters, c->qs.eng.d_after_lo, excl_arg(c));
        });
    });
}

// optimized_parallel.hpp:67: const uint32_t sn = uint32_t(sample_proportion * n);  (float product)
uint32_t sample_rows(float sample_proportion, uint32_t n)
{
    const float p = sample_proportion * (float)n;
    if (!(p > 0.0f)) return 0u;
    if (p >= 4294967296.0f) return n;
    const uint32_t sn = (uint32_t)p;
    return sn > n ? n : sn;
}

int ensure_results(hvs_ctx* c, uint32_t nq)
{
    if (nq <= c->res_cap) return HVS_OK;
    int rc;
    if ((rc = dev_alloc(c, &c->d_out_ids, (size_t)nq * c->k))) return rc;
    if ((rc = dev_alloc(c, &c->d_out_dists, (size_t)nq * c->k))) return rc;
    if ((rc = dev_alloc(c, &c->call.d_ovf_list, (size_t)nq))) return rc;
    if ((rc = dev_alloc(c, &c->call.d_retry_list, (size_t)nq))) return rc;
    c->res_cap = nq;
    return HVS_OK;
}

int ensure_queries(hvs_ctx* c, uint32_t nq)
{
    if (nq > c->nq_cap) {
        int rc;
        c->nq_cap = 0;  // (the two buffers grow together: a failure between them leaves neither in use)
        if ((rc = dev_alloc(c, &c->d_q, (size_t)nq * HVS_QCOLS))) return rc;
        if ((rc = per_query_room(c, c->qs.eng, kCaps, nq))) return rc;
        c->nq_cap = nq;
    }
    return ensure_results(c, nq);
}

struct Plan {
    uint32_t nq_pad, qwaves, nchunks, rows_per_chunk;
};

Plan make_plan(uint32_t nqb, uint32_t sn)
{
    Plan p;
    p.qwaves = (nqb + 63u) / 64u;
    p.nq_pad = ((nqb + 255u) / 256u) * 256u;
    // enough (query-wave x row-chunk) work items to fill 256 CUs x 16 waves, but chunks of >= 2048 rows
    uint32_t want = (8192u + p.qwaves - 1u) / p.qwaves;
    uint32_t max_chunks = std::max(1u, sn / 2048u);
    // (a handful of queries -- the filter engines' fallback list -- is one wave per chunk: up to 512 chunks then, so that
    // a single query does not walk 10^7 rows with 64 waves)
    p.nchunks = std::max(1u, std::min(std::min(want, max_chunks), p.qwaves <= 2u ? 512u : 64u));
    p.rows_per_chunk = (sn + p.nchunks - 1u) / p.nchunks;
    if (p.rows_per_chunk == 0) p.rows_per_chunk = 1;
    return p;
}

int ensure_batch_workspace(hvs_ctx* c, uint32_t nqb, const Plan& p)
{
    int rc;
    if (nqb > c->batch_cap) {
        if ((rc = dev_alloc(c, &c->d_keys, (size_t)nqb))) return rc;
        if ((rc = dev_alloc(c, &c->d_keys_sorted, (size_t)nqb))) return rc;
        if ((rc = dev_alloc(c, &c->d_qidx, (size_t)nqb))) return rc;
        if ((rc = dev_alloc(c, &c->d_qorder, (size_t)nqb))) return rc;
        if ((rc = dev_alloc(c, &c->d_qra, (size_t)nqb))) return rc;
        if ((rc = dev_alloc(c, &c->d_qrb, (size_t)nqb))) return rc;
        size_t tmp = 0;
        HVS_HIP(c, rocprim::radix_sort_pairs(nullptr, tmp, c->d_keys, c->d_keys_sorted, c->d_qidx, c->d_qorder,
                                             (size_t)nqb, 0, 64, c->stream));
        if (tmp > c->sort_tmp_bytes) {
            if (c->d_sort_tmp) (void)hipFree(c->d_sort_tmp);
            c->d_sort_tmp = nullptr;
            HVS_HIP(c, hipMalloc(&c->d_sort_tmp, tmp));
            c->sort_tmp_bytes = tmp;
        }
        c->batch_cap = nqb;
    }
    const size_t lists = (size_t)p.nq_pad * p.nchunks;
    if (lists > c->cand_lists) {
        if ((rc = dev_alloc(c, &c->d_cand, lists * (size_t)c->cap))) return rc;
        if ((rc = dev_alloc(c, &c->d_cand_cnt, lists))) return rc;
        c->cand_lists = lists;
    }
    return HVS_OK;
}

// One batch of resident queries through the exact engine.  Either the contiguous range
// [q0, q0+nqb) (sorted into predicate groups first) or, when `list` is given, the nqb query
// indices stored in the device array `list` (the MFMA engine's overflow fallback).
int run_batch_exact(hvs_ctx* c, uint32_t q0, uint32_t nqb, uint32_t sn, const uint32_t* list = nullptr,
                    bool count_stats = true, bool record_events = true)
{
    const Plan p = make_plan(nqb, sn);
    int rc = ensure_batch_workspace(c, nqb, p);
    if (rc) return rc;

    const uint32_t* qorder = list;
    if (!list) {
        hipLaunchKernelGGL(hvs_k_query_keys, dim3((nqb + 255u) / 256u), dim3(256), 0, c->stream, c->d_q, q0, nqb,
                           c->d_keys, c->d_qidx);
        size_t tmp = c->sort_tmp_bytes;
        HVS_HIP(c, rocprim::radix_sort_pairs(c->d_sort_tmp, tmp, c->d_keys, c->d_keys_sorted, c->d_qidx, c->d_qorder,
                                             (size_t)nqb, 0, 64, c->stream));
        qorder = c->d_qorder;
    }
    HVS_HIP(c, hipMemsetAsync(c->d_cand_cnt, 0, (size_t)p.nq_pad * p.nchunks * sizeof(uint32_t), c->stream));

    const int ev = record_events ? kernel_timer_begin(c) : -1;
    if (sn > 0) {
        unsigned long long* stat = exact_batch_counters(c, count_stats);
        const dim3 grid(p.nq_pad / 256u, p.nchunks);
        with_order_cap_mask(c, [&](auto ST, auto CAPT, auto MT) {
            with_capped_after(c, [&](auto WT, auto AT, auto XT) {
                hipLaunchKernelGGL(
                    (hvs_k_scan_exact_lds<decltype(ST)::value, decltype(CAPT)::value, decltype(MT)::value, decltype(WT)::value, decltype(AT)::value, decltype(XT)::value>),
                    grid, dim3(256), 0, c->stream, c->d_data, c->d_q, qorder, nqb, p.nq_pad, sn, p.rows_per_chunk, c->d_cand, c->d_cand_cnt, stat,
                    c->k, c->rs.d_live, c->qs.eng.d_max_d2, c->qs.eng.d_after_lo, excl_arg(c));
            });
        });
    }
    kernel_timer_end(c, ev);
    launch_select(c, qorder, nqb, p.nq_pad, p.nchunks, c->d_cand, c->d_cand_cnt);
    HVS_HIP(c, hipGetLastError());
    return HVS_OK;
}

// ---------------------------------------------------------------------------------------------
// MFMA engine: index build
// ---------------------------------------------------------------------------------------------
void free_index(hvs_ctx* c)
{
    for (HvsOrdering& o : c->ord) {
        void* ptrs[] = {o.keys, o.perm, o.tiles, o.nrm, o.bpos};
        for (void* p : ptrs)
            if (p) (void)hipFree(p);
        uint32_t* lp = o.lp;  // (the live-row counts' buffer outlives the index)
        o = HvsOrdering{};
        o.lp = lp;
    }
    c->have_order = false;
    c->n_indexed = 0;
    c->rs.lp_valid = false;  // (counts along the orderings that have just gone)
    // everything the last data set taught, `planned` and `built_rot` included: nothing reads those two before choose_format
    // and build_tiles have written them for the next index
    c->fmt = HvsFormatState{};
}

// Planner of HVS_ENGINE_AUTO, first guess: which tile format filters this data set more cheaply.  The INT8 filter runs
// at about twice the tile rate of the 16-bit float filters (profiles/) but its error band can be wider, and the FP16
// band is 8x tighter than the BF16 one at the same cost; a wider band inflates the number of survivors the exact kernel
// re-scores by about exp(z * 2 band / sigma): sigma = spread of squared distances between rows, z = how many sigmas
// below the mean the k-th neighbour of n rows sits.  Everything here is an estimate from a sample of rows and a
// unimodal model of the distances -- build_index checks the choice with a probe batch (probe_format) -- and it decides
// speed only: all formats give the same answers.
// HVS_I8_ROTATE: 0 = INT8 tiles never rotated, 1 = always (HVS_FMT_I8X16), unset = the planner's probe decides (read per
// data set, so that a test can switch it between contexts)
int rotate_policy()
{
    const char* v = std::getenv("HVS_I8_ROTATE");
    if (!v || !*v) return -1;
    return std::atoi(v) != 0 ? 1 : 0;
}

// HVS_FILTER_FORMAT = "bf16" / "f16" / "i8": A/B override of the planner; set to anything, it also switches the probe off
// (read per data set, like HVS_I8_ROTATE)
const char* forced_format() { return std::getenv("HVS_FILTER_FORMAT"); }
// HVS_PLAN_BF16_COST: what a 16-bit float filter launch costs in hundredths of an INT8 one, for the model and for the probe
double plan_cost16() { return env_u32("HVS_PLAN_BF16_COST", 194u, 100u, 1000u) / 100.0; }

// centre and scale of the INT8 format over the vector components (`rot` false) or over their rotated images (HvsQuant)
int set_quant(hvs_ctx* c, bool rot)
{
    if (!c->d_quant) HVS_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->d_quant), sizeof(HvsQuant)));
    hipLaunchKernelGGL(hvs_k_quant_reset, dim3(1), dim3(128), 0, c->stream, c->d_quant, rot ? 1u : 0u);
    if (rot)
        hipLaunchKernelGGL(hvs_k_minmax_rot, dim3(std::min(c->n_indexed, 4096u)), dim3(128), 0, c->stream, c->d_data, c->n_indexed, c->d_quant);
    else
        hipLaunchKernelGGL(hvs_k_minmax, dim3(std::min(c->n_indexed, 4096u)), dim3(128), 0, c->stream, c->d_data, c->n_indexed, c->d_quant);
    hipLaunchKernelGGL(hvs_k_quant_params, dim3(1), dim3(128), 0, c->stream, c->d_quant);
    HVS_HIP(c, hipGetLastError());
    c->fmt.i8_rot = rot;
    return HVS_OK;
}

int choose_format(hvs_ctx* c)
{
    const uint32_t n = c->n_indexed;
    c->fmt.planned = HVS_FMT_F16;
    c->fmt.i8_usable = false;
    int rcq = set_quant(c, false);  // (the model below prices the plain INT8 format; HVS_I8_ROTATE=1 switches afterwards)
    if (rcq) return rcq;
    if (!c->d_bounds) HVS_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->d_bounds), sizeof(HvsBounds)));
    HVS_HIP(c, hipMemsetAsync(c->d_bounds, 0, sizeof(HvsBounds), c->stream));
    const uint32_t step = std::max(1u, n / 65536u);
    const uint32_t samples = hvs_ceil_div(n, step);
    hipLaunchKernelGGL(hvs_k_plan_stats, dim3(hvs_ceil_div(samples, 256u)), dim3(256), 0, c->stream, c->d_data, n, step,
                       c->d_quant, c->d_bounds);
    HVS_HIP(c, hipGetLastError());
    HvsBounds hb{};
    double sd = 0.0;
    HVS_HIP(c, hipMemcpyAsync(&hb, c->d_bounds, sizeof(hb), hipMemcpyDeviceToHost, c->stream));
    HVS_HIP(c, hipMemcpyAsync(&sd, reinterpret_cast<const char*>(c->d_quant) + offsetof(HvsQuant, sd), sizeof(double),
                              hipMemcpyDeviceToHost, c->stream));
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    c->fmt.i8_usable = sd > 0.0 && std::isfinite(sd);
    const bool f16_ok = std::isfinite(hb.nb_df) && std::isfinite(hb.e_df) && hb.hmax < 3.0e4f;
    if (!f16_ok) c->fmt.planned = HVS_FMT_BF16;
    if (hb.pair_n >= 16u) {
        const double mean = hb.pair_sum / hb.pair_n;
        const double var = hb.pair_sumsq / hb.pair_n - mean * mean;
        const double sigma = std::sqrt(std::max(var, 1e-300));
        // z of the k-th neighbour among n rows (normal tail, crude): k/n = Phi(-z)
        const double pq = std::min(0.4, (double)c->k / (double)n);
        const double z = std::sqrt(std::max(0.0, -2.0 * std::log(pq) - std::log(-2.0 * std::log(pq) * 6.2832)));
        // bands for a query that looks like a row (|q| ~ row norm, quantisation error ~ row error)
        const double acc16 = 4.0e-5 * ((double)hb.nb_d * (double)hb.nb_d + (double)hb.hmax);
        const double band_bf = 2.0 * (double)hb.nb_d * (double)hb.e_d + acc16;
        const double band_f = 2.0 * (double)hb.nb_df * (double)hb.e_df + acc16;
        const double band8 = 2.0 * (double)hb.n_d8 * (double)hb.e_d8;
        const double infl_bf = std::exp(std::min(50.0, z * 2.0 * band_bf / sigma));
        const double infl_f = std::exp(std::min(50.0, z * 2.0 * band_f / sigma));
        const double infl8 = std::exp(std::min(50.0, z * 2.0 * band8 / sigma));
        // cost model in units of one INT8 filter launch: a 16-bit float filter takes kPlan16 times as long, re-scoring
        // kPlanRescore times at inflation 1 and grows with the candidates (HVS_PLAN_BF16_COST / HVS_PLAN_RESCORE_COST, in
        // hundredths, override the measured defaults of profiles/)
        const double kPlan16 = plan_cost16();
        const double kPlanRescore = env_u32("HVS_PLAN_RESCORE_COST", 15u, 1u, 1000u) / 100.0;
        const double cost_f = kPlan16 + kPlanRescore * (f16_ok ? infl_f : infl_bf), cost8 = 1.0 + kPlanRescore * infl8;
        if (c->fmt.i8_usable && cost8 < cost_f && infl8 < 6.0) c->fmt.planned = kI8Fmt;
    }
    if (const char* f = forced_format()) {
        if (!std::strcmp(f, "bf16")) c->fmt.planned = HVS_FMT_BF16;
        if (!std::strcmp(f, "f16")) c->fmt.planned = HVS_FMT_F16;
        if (!std::strcmp(f, "i8")) c->fmt.planned = kI8Fmt;
    }
    if (rotate_policy() == 1 && kI8Fmt == HVS_FMT_I8X16 && c->fmt.i8_usable) {
        if ((rcq = set_quant(c, true))) return rcq;
        double sdr = 0.0;
        HVS_HIP(c, hipMemcpyAsync(&sdr, reinterpret_cast<const char*>(c->d_quant) + offsetof(HvsQuant, sd), sizeof(double),
                                  hipMemcpyDeviceToHost, c->stream));
        HVS_HIP(c, hipStreamSynchronize(c->stream));
        if (!(sdr > 0.0 && std::isfinite(sdr)) && (rcq = set_quant(c, false))) return rcq;
    }
    return HVS_OK;
}

// hvs_timing.pairs under a mask: live rows in front of every position of both orderings (see hvs_k_live_flags); made on first
// use after a mask change
int ensure_live_prefix(hvs_ctx* c)
{
    if (c->rs.lp_valid) return HVS_OK;
    const uint32_t n = c->n_indexed;  // (positions)
    int rc;
    for (HvsOrdering& o : c->ord)
        if (!o.lp && (rc = dev_alloc(c, &o.lp, (size_t)n + 1u))) return rc;
    size_t tmp_bytes = 0;
    HVS_HIP(c, rocprim::exclusive_scan(nullptr, tmp_bytes, c->ord[0].lp, c->ord[0].lp, 0u, (size_t)n + 1u, rocprim::plus<uint32_t>(), c->stream));
    void* tmp = nullptr;
    HVS_HIP(c, hipMalloc(&tmp, tmp_bytes ? tmp_bytes : 1));
    hipError_t e = hipSuccess;
    for (const HvsOrdering& o : c->ord) {
        if (e != hipSuccess) break;
        hipLaunchKernelGGL(hvs_k_live_flags, dim3(hvs_ceil_div(n + 1u, 256u)), dim3(256), 0, c->stream, index_mask(c), o.perm, n, o.lp);
        e = rocprim::exclusive_scan(tmp, tmp_bytes, o.lp, o.lp, 0u, (size_t)n + 1u, rocprim::plus<uint32_t>(), c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(tmp);
    if (e != hipSuccess) return fail(c, HVS_EHIP, std::string("live-row counts: ") + hipGetErrorString(e));
    c->rs.lp_valid = true;
    return HVS_OK;
}

// passing pairs of a batch under a mask (HVS_CNT_PAIRS): from the prefix counts, or row by row when a sampled prefix cuts in
int count_masked_pairs(hvs_ctx* c, uint32_t sn)
{
    HvsBatch& B = c->fb;
    if (sn >= c->n_indexed) {  // (no indexed row is cut off)
        int rc = ensure_live_prefix(c);
        if (rc) return rc;
        hipLaunchKernelGGL(hvs_k_count_live_pairs, dim3(hvs_ceil_div(B.nslots, 256u)), dim3(256), 0, c->stream, B, c->ord[0].lp, c->ord[1].lp,
                           c->call.d_counters);
    } else {
        hipLaunchKernelGGL(hvs_k_count_prefix_pairs<true>, dim3(B.nslots), dim3(64), 0, c->stream, B, c->ord[0].perm, c->ord[1].perm, sn,
                           c->call.d_counters, index_mask(c));
    }
    return HVS_OK;
}

// Tombstones (hvs_k_patch_tiles): the never-hit encoding over the tile entries of the dead and the stale rows, both orderings.
// Called after every mask change that only kills rows, after every update that makes rows stale, and at the end of every tile
// build while rows are dead or stale.
int patch_tiles(hvs_ctx* c)
{
    if (!masked(c) || c->fmt.built == HVS_FMT_NONE || !c->ord[0].tiles || !index_mask(c) || !c->rs.d_mask_stat) return HVS_OK;
    const HvsLevels L = c->lv;
    HVS_HIP(c, hipMemsetAsync(c->rs.d_mask_stat, 0, 2 * sizeof(unsigned long long), c->stream));
    const dim3 grid((L.nblk + 3u) / 4u);
    for (const HvsOrdering& o : c->ord)
        hipLaunchKernelGGL(hvs_k_patch_tiles, grid, dim3(256), 0, c->stream, index_mask(c), o.perm, c->n_indexed, L, o.bpos, o.tiles,
                           reinterpret_cast<int*>(o.nrm), c->fmt.built, c->rs.d_mask_stat);
    HVS_HIP(c, hipGetLastError());
    return HVS_OK;
}

// (re)build the level-interleaved tiles of both orderings in format `fmt`; the orderings must exist.  An unusable bound is no
// error: fmt.built stays HVS_FMT_NONE
int build_tiles(hvs_ctx* c, int fmt)
{
    const HvsLevels L = c->lv;
    const uint32_t n = c->n_indexed;
    int rc;
    c->fmt.built = HVS_FMT_NONE;
    if (c->rs.d_mask_stat) HVS_HIP(c, hipMemsetAsync(c->rs.d_mask_stat, 0, 2 * sizeof(unsigned long long), c->stream));  // fresh tiles: none patched
    // free first: the two formats never coexist (D = 1e8: 44.8 GB of BF16 tiles, 20.8 GB of INT8 tiles)
    for (HvsOrdering& o : c->ord) {
        if ((rc = dev_alloc(c, &o.tiles, (size_t)0))) return rc;
        if ((rc = dev_alloc(c, &o.nrm, (size_t)0))) return rc;
    }
    const HvsHostFmt F = hvs_host_fmt(fmt, c->fmt.i8_rot);
    for (HvsOrdering& o : c->ord) {
        if ((rc = dev_alloc(c, &o.tiles, (size_t)L.nblk * F.tile_u4))) return rc;
        if (F.nrm_u4 && (rc = dev_alloc(c, &o.nrm, (size_t)L.nblk * F.nrm_u4))) return rc;
        if (!o.bpos && (rc = dev_alloc(c, &o.bpos, (size_t)L.nblk))) return rc;
    }
    HVS_HIP(c, hipMemsetAsync(c->d_bounds, 0, sizeof(HvsBounds), c->stream));
    const dim3 grid((L.nblk + 3u) / 4u);
    for (const HvsOrdering& o : c->ord) {
        if (F.build_i8)
            hipLaunchKernelGGL(F.build_i8, grid, dim3(256), 0, c->stream, c->d_data, n, o.perm, L, c->d_quant, o.tiles,
                               reinterpret_cast<int*>(o.nrm), o.bpos, c->d_bounds);
        else
            hipLaunchKernelGGL(hvs_k_build_tiles, grid, dim3(256), 0, c->stream, c->d_data, n, o.perm, L, o.tiles, o.bpos, c->d_bounds, fmt);
    }
    HVS_HIP(c, hipGetLastError());
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    HvsBounds hb{};
    HVS_HIP(c, hipMemcpy(&hb, c->d_bounds, sizeof(hb), hipMemcpyDeviceToHost));
    const bool ok = hvs_bounds_usable(fmt, hb);
    if (kTrace)
        std::fprintf(stderr, "[hvs trace] tiles built: format %d usable %d e_d8 %.6g n_d8 %.6g e_d %.6g nb_d %.6g hmax %.6g rho %.6g\n", fmt, (int)ok,
                     (double)hb.e_d8, (double)hb.n_d8, (double)hb.e_d, (double)hb.nb_d, (double)hb.hmax, (double)hb.rho);
    if (!ok) return HVS_OK;
    c->fmt.built = fmt;
    c->fmt.built_rot = HVS_IS_I8(fmt) && c->fmt.i8_rot;
    return patch_tiles(c);  // (nothing while every row is live)
}

int run_batch_mfma(hvs_ctx* c, uint32_t q0, uint32_t nqb, uint32_t sn, const uint32_t* list, bool proven_last, BatchGates gates = {});
HvsGuessTable plan_guess(uint32_t k, bool proven, uint32_t pfail);

bool is_filter_engine(int engine) { return engine == HVS_ENGINE_MFMA_FILTER || engine == HVS_ENGINE_MFMA_I8 || engine == HVS_ENGINE_MFMA_F16; }
// the engine setting asks for a filter: forced, or HVS_ENGINE_AUTO on a data set the planner found one for (the callers add
// what else they need: orderings, the sampled prefix, the summation order)
bool filter_engine_selected(const hvs_ctx* c)
{
    return is_filter_engine(c->engine) || (c->engine == HVS_ENGINE_AUTO && c->n >= kMfmaMinRows && c->fmt.planned != HVS_FMT_NONE);
}

// The precision chain INT8 -> FP16 -> BF16: the next format below `fmt` that this data set has not rejected (HVS_FMT_NONE
// below BF16, the last resort, which is built whatever happened to it before)
int next_format_down(const hvs_ctx* c, int fmt)
{
    if (HVS_IS_I8(fmt) && !c->fmt.f16_rejected) return HVS_FMT_F16;
    return fmt == HVS_FMT_BF16 ? HVS_FMT_NONE : HVS_FMT_BF16;
}

// the tile format the context's engine setting asks for (HVS_FMT_NONE: HVS_ENGINE_AUTO found no filter worth running)
int want_format(const hvs_ctx* c)
{
    int want;
    switch (c->engine) {
        case HVS_ENGINE_MFMA_FILTER: want = HVS_FMT_BF16; break;
        case HVS_ENGINE_MFMA_F16: want = HVS_FMT_F16; break;
        case HVS_ENGINE_MFMA_I8: want = c->fmt.i8_usable ? kI8Fmt : HVS_FMT_F16; break;
        default: want = c->fmt.planned; break;
    }
    const bool rejected = HVS_IS_I8(want) ? c->fmt.i8_rejected : (want == HVS_FMT_F16 && c->fmt.f16_rejected);
    return rejected ? next_format_down(c, want) : want;
}

// build `want`, or the next format down the chain whose bound is usable on this data set (fmt.built stays HVS_FMT_NONE when
// none is)
int build_tiles_chain(hvs_ctx* c, int want)
{
    for (; want != HVS_FMT_NONE; want = next_format_down(c, want)) {
        int rc = build_tiles(c, want);
        if (rc) return rc;
        if (c->fmt.built != HVS_FMT_NONE) return HVS_OK;
        if (HVS_IS_I8(want)) c->fmt.i8_rejected = true;
        if (want == HVS_FMT_F16) c->fmt.f16_rejected = true;
    }
    return HVS_OK;
}

// Planner of HVS_ENGINE_AUTO, second step: measure instead of model.  A probe batch of 1024 rows of D used as type-0
// queries (only D is used, cf. README.md:68) runs through the filter engine in the format just built; what it hands to the
// exact kernel and what it cannot answer is priced in units of the INT8 filter's own time per query:
//     cost = F + (2650 / n) re-scored pairs per query + 3 retried fraction + 142 exact-engine fraction
// (F = 1 for INT8 tiles, 1.94 for 16-bit float tiles; re-scoring 0.07 ns per pair against 0.0266 ns per row and query of the
// INT8 filter, the exact engine 140x the filter -- profiles/r03), next to its INFLATION = re-scored pairs / what a filter
// without an error band would hand over under the same guessed thresholds, and the fraction of queries it left unanswered.  The model of choose_format assumes one bell-shaped
// distance distribution; clustered data and data with a few dominant dimensions have neighbour distances far below what
// it expects, and an 8-bit grid over the bounding box then lets thousands of rows per query through.
int probe_format(hvs_ctx* c, double* cost, double* inflation, double* failed)
{
    constexpr uint32_t P = 1024;
    *cost = 1.0e9;
    if (c->call.pending) return fail(c, HVS_ESTATE, "internal: planner probe while a call's re-runs are pending");  // (h_ovf and the counts are that call's)
    // the probe has its own query / result / re-run buffers, in the context's fields while it runs: resident queries and
    // results of the caller stay untouched
    ScopedDevBufs own;
    if (own.lend(&c->d_q, (size_t)P * HVS_QCOLS) != hipSuccess || own.lend(&c->d_out_dists, (size_t)P * c->k) != hipSuccess ||
        own.lend(&c->d_out_ids, (size_t)P * c->k) != hipSuccess || own.lend(&c->call.d_ovf_list, (size_t)P) != hipSuccess ||
        own.lend(&c->call.d_retry_list, (size_t)P) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, HVS_ENOMEM, "planner probe: out of device memory");
    }
    // (rows of the indexed part, searched in the indexed part: the probe prices the index, and runs when it covers every row)
    const uint32_t step = std::max(1u, c->n_indexed / P);
    hipLaunchKernelGGL(hvs_k_probe_queries, dim3(hvs_ceil_div(P * HVS_QCOLS, 256u)), dim3(256), 0, c->stream, c->d_data, c->n_indexed, step, P, c->d_q);
    // (the probe batch is small, but it stands for full batches: their failure target.  Its lists keep the production capacity:
    // PCA-like vectors at n = 10^7 hand ~1500 rows per type-0 query to the last level's list of 1024 -- INT8 tiles look 23 %
    // faster than FP16 tiles there only while a half-empty workspace doubles the lists, profiles/r04/nonuniform_int8.txt)
    c->force_pfail = guess_pfail_for(kBatchMfma);
    int rc = counters_begin(c);
    if (!rc) {
        const DetachedForProbe probe(c->qs);
        rc = run_batch_mfma(c, 0, P, c->n_indexed, nullptr, false);
    }
    c->force_pfail = 0u;
    unsigned long long rescored[1] = {0};
    uint32_t fails[2] = {0, 0};
    if (!rc) rc = fetch_fail_counts(c, &fails[0], &fails[1]);  // (waits for the batch)
    if (!rc) rc = call_counters(c, HVS_CNT_RESCORED, rescored, true);
    if (rc) (void)hipStreamSynchronize(c->stream);  // (the lent buffers go when this returns)
    call_forgotten(c);
    if (rc) return rc;
    const double base = HVS_IS_I8(c->fmt.built) ? 1.0 : plan_cost16();
    *cost = base + 2650.0 / (double)c->n_indexed * ((double)rescored[0] / P) + 3.0 * fails[1] / P + 142.0 * fails[0] / P;
    // what a filter without any error band would have handed over: m (radix - 1) rows per level under the guessed thresholds
    double ideal = 0.0;
    {
        const HvsGuessTable G = plan_guess(c->k, false, guess_pfail_for(kBatchMfma));
        double seen = 1.0;  // fraction of the rows seen, from the last level backwards
        for (uint32_t j = c->lv.K; j >= 1u; --j) {
            seen /= (double)c->lv.radix[j];
            int idx = (int)std::ceil(8.0 * -std::log2(seen) - 0.02);
            idx = std::max(0, std::min(HVS_GUESS_STEPS - 1, idx));
            const double m = G.last_m && j == c->lv.K ? (double)G.last_m : (double)std::max(G.m[idx], G.floor_m);
            ideal += std::min(m, (double)c->k) * ((double)c->lv.radix[j] - 1.0);
        }
    }
    *inflation = ideal > 0.0 ? ((double)rescored[0] / P) / ideal : 1.0;
    *failed = (double)(fails[0] + fails[1]) / P;
    return HVS_OK;
}

// after build_tiles_chain in HVS_ENGINE_AUTO: keep the format the model chose if the probe agrees, else try the next one up
// the precision chain; planned_fmt = HVS_FMT_NONE when no filter beats the exact engine
int plan_by_probe(hvs_ctx* c)
{
    if (!env_u32("HVS_PLAN_PROBE", 1u, 0u, 1u) || forced_format()) return HVS_OK;
    // probe the tiles that are built and say so in the trace (`ok` stays false when none are: nothing to compare)
    struct Probed {
        bool ok = false;
        double cost = 0.0, infl = 0.0, failed = 0.0;
    } p;
    auto probe = [&](const char* tag) -> int {
        p = Probed{};
        if (c->fmt.built == HVS_FMT_NONE) return HVS_OK;
        const int rc = probe_format(c, &p.cost, &p.infl, &p.failed);
        if (rc) return rc;
        p.ok = true;
        if (kTrace)
            std::fprintf(stderr, "[hvs trace] planner probe: format %d%s cost %.3f inflation %.2f failed %.4f\n", c->fmt.built, tag, p.cost, p.infl,
                         p.failed);
        return HVS_OK;
    };
    int rc = probe("");
    if (rc) return rc;
    int best = c->fmt.built;
    bool best_rot = c->fmt.i8_rot;
    double best_cost = p.cost;
    // INT8 tiles stay unless their band visibly lets too much through on this data (the cost formula is not trusted to
    // split hairs between formats that both work: at small n everything is launch latency).  Otherwise the candidates are
    // probed in turn -- the rotated INT8 tiles (same filter rate; HvsQuant), then the FP16 tiles (half the rate, an 8x tighter
    // band) -- and the cheapest stays.
    if (HVS_IS_I8(c->fmt.built) && (p.infl > 2.5 || p.failed > 0.01)) {
        const int had = c->fmt.built;
        if (had == HVS_FMT_I8X16 && !c->fmt.i8_rot && rotate_policy() != 0) {
            if ((rc = set_quant(c, true))) return rc;
            if ((rc = build_tiles(c, had))) return rc;
            if ((rc = probe(" (rotated)"))) return rc;
            if (p.ok && p.cost < best_cost) {
                best_rot = true;
                best_cost = p.cost;
            }
        }
        if (!c->fmt.f16_rejected) {
            if ((rc = build_tiles_chain(c, HVS_FMT_F16))) return rc;
            if ((rc = probe(""))) return rc;
            if (p.ok && p.cost < best_cost) {
                best = c->fmt.built;
                best_cost = p.cost;
            }
        }
        if (HVS_IS_I8(best)) {  // an INT8 variant stays: its centre / scale and tiles come back if something else was built last
            if (c->fmt.i8_rot != best_rot && (rc = set_quant(c, best_rot))) return rc;
            if ((c->fmt.built != best || c->fmt.built_rot != best_rot) && (rc = build_tiles_chain(c, had))) return rc;
        } else if (c->fmt.i8_rot && (rc = set_quant(c, false))) {  // (a later change of engine finds the plain INT8 parameters)
            return rc;
        }
    }
    if (best_cost >= 140.0) best = HVS_FMT_NONE;  // no filter beats the exact engine's range scans here
    c->fmt.planned = best;
    return HVS_OK;
}

// keys and perm of both orderings: two radix sorts over temporaries that go when this returns
int build_orderings(hvs_ctx* c)
{
    const uint32_t n = c->n_indexed;
    int rc;
    for (HvsOrdering& o : c->ord) {
        if ((rc = dev_alloc(c, &o.keys, (size_t)n))) return rc;
        if ((rc = dev_alloc(c, &o.perm, (size_t)n))) return rc;
    }
    ScopedDevBufs temps;
    uint64_t *k_ct = nullptr, *k_t = nullptr;
    uint32_t* ids = nullptr;
    char* tmp = nullptr;
    HVS_HIP(c, temps.alloc(&k_ct, (size_t)n));
    HVS_HIP(c, temps.alloc(&k_t, (size_t)n));
    HVS_HIP(c, temps.alloc(&ids, (size_t)n));
    hipLaunchKernelGGL(hvs_k_attr_keys, dim3((n + 255u) / 256u), dim3(256), 0, c->stream, c->d_data, n, k_ct, k_t, ids);
    size_t tmp_bytes = 0, tmp_bytes_t = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, tmp_bytes, k_ct, c->ord[0].keys, ids, c->ord[0].perm, (size_t)n, 0, 64,
                                             c->stream);
    if (e == hipSuccess)
        e = rocprim::radix_sort_pairs(nullptr, tmp_bytes_t, k_t, c->ord[1].keys, ids, c->ord[1].perm, (size_t)n, 0, 64, c->stream);
    if (tmp_bytes_t > tmp_bytes) tmp_bytes = tmp_bytes_t;  // each call sizes its own algorithm
    if (e == hipSuccess) e = temps.alloc(&tmp, tmp_bytes);
    if (e == hipSuccess)
        e = rocprim::radix_sort_pairs(tmp, tmp_bytes, k_ct, c->ord[0].keys, ids, c->ord[0].perm, (size_t)n, 0, 64, c->stream);
    if (e == hipSuccess)
        e = rocprim::radix_sort_pairs(tmp, tmp_bytes, k_t, c->ord[1].keys, ids, c->ord[1].perm, (size_t)n, 0, 64, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, e == hipErrorOutOfMemory ? HVS_ENOMEM : HVS_EHIP, std::string("index sort: ") + hipGetErrorString(e));
    c->have_order = true;
    return HVS_OK;
}

int build_index(hvs_ctx* c)
{
    free_index(c);
    const uint32_t n = c->n;  // an index is always built over every row there is
    const HvsLevels L = hvs_make_levels(n, kRadixLast, kRadixMid, kRadixPlan.set ? kRadixPlan.r : nullptr);
    if (L.off[L.K + 1] != L.nblk) return fail(c, HVS_EINVAL, "internal: level table does not cover the blocks");
    // survivor entries carry the block position in 24 bits: above 2^29 rows per GPU the exact engine answers
    // (2^29 rows are 219 GB of rows alone: such a data set is sharded over GPUs anyway)
    c->index_too_large = L.nblk > HVS_ENTRY_MAX_BLOCKS;
    if (c->index_too_large) return HVS_OK;
    c->lv = L;
    c->n_indexed = n;  // (free_index takes it back when the build fails)
    int rc = build_orderings(c);
    trace_mark(c, "orderings");
    if (!rc) rc = choose_format(c);
    trace_mark(c, "format");
    if (!rc) rc = build_tiles_chain(c, want_format(c));  // (choose_format always plans a format)
    trace_mark(c, "tiles");
    if (!rc && c->fmt.built != HVS_FMT_NONE && c->engine == HVS_ENGINE_AUTO && n >= kMfmaMinRows) {
        rc = plan_by_probe(c);
        trace_mark(c, "probe");
    }
    // An error leaves no half-built index behind.  Nor does a data set on which no format has a usable bound (non-finite
    // components, norms out of range): at load time the orderings go as well and the exact engine scans without ranges
    // 
    if (rc || c->fmt.built == HVS_FMT_NONE) free_index(c);
    return rc;
}

// ---------------------------------------------------------------------------------------------
// MFMA engine: one batch
// ---------------------------------------------------------------------------------------------
// `want_fcap`: candidate keys per slot and round the batch needs (HVS_FCAP for ordinary batches; retry batches, which run
// every level with the proven threshold, ask for more); the lists take whatever the workspace offers beyond that
int ensure_filter_workspace(hvs_ctx* c, uint32_t nqb, uint32_t want_fcap = HVS_FCAP)
{
    const uint32_t slots = hvs_ceil_div(nqb + 5u * 32u + (HVS_WG_WAVES + 1u) * HVS_GROUP, HVS_GROUP) * HVS_GROUP;
    const uint32_t groups = slots / HVS_GROUP;
    if (slots > HVS_ENTRY_MAX_SLOTS) return fail(c, HVS_EINVAL, "internal: batch too large for the survivor entries' slot field");
    HvsBatch& B = c->fb;
    int rc;
    if (slots > c->fb_slots_cap) {
        c->fb_slots_cap = 0;  // (a failed allocation below leaves no half-sized workspace behind)
#define HVS_A(field, count) \
    if ((rc = dev_alloc(c, &B.field, (size_t)(count)))) return rc
        HVS_A(qid, slots);
        HVS_A(rank, slots);
        HVS_A(ra, slots);
        HVS_A(rb, slots);
        HVS_A(gua, groups);
        HVS_A(gub, groups);
        HVS_A(gord, groups);
        HVS_A(bfrag, (size_t)(slots / 32u) * HVS_TILE_U4);
        HVS_A(theta, slots);
        B.thetai = reinterpret_cast<int*>(B.theta);
        HVS_A(qn, slots);
        HVS_A(normq, slots);
        HVS_A(eq, slots);
        HVS_A(nqb, slots);
        HVS_A(top, (size_t)slots * 256u);  // stride 128 (k <= 128) or 256
        HVS_A(topcnt, slots);
        HVS_A(tau, slots);
        HVS_A(candcnt, slots);
        HVS_A(overflow, slots);
        HVS_A(paircnt, groups);
        HVS_A(goverflow, groups);
#undef HVS_A
        if (!c->d_layout) HVS_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->d_layout), 16 * sizeof(uint32_t)));
        c->fb_slots_cap = slots;
    }
    // candidate lists and survivor-entry lists: sized in entries, shared out over the slots / groups of the batch
    const size_t need_cand = (size_t)slots * want_fcap, need_pairs = (size_t)groups * HVS_GROUP * want_fcap;
    if (need_cand > c->fb_cand_entries) {
        c->fb_cand_entries = 0;  // (dev_alloc releases the old buffer first: nothing is held if it fails)
        if ((rc = dev_alloc(c, &B.cand, need_cand))) return rc;
        c->fb_cand_entries = need_cand;
    }
    if (need_pairs > c->fb_pair_entries) {
        c->fb_pair_entries = 0;
        if ((rc = dev_alloc(c, &B.pairs, need_pairs))) return rc;
        c->fb_pair_entries = need_pairs;
    }
    B.nslots = slots;
    B.ngroups = groups;
    B.fcap = (uint32_t)std::min<size_t>(16384u, c->fb_cand_entries / slots);
    B.gcap = (uint32_t)std::min<size_t>((size_t)HVS_GROUP * 16384u, c->fb_pair_entries / groups);
    if (c->force_pfail) {  // planner probe: a full batch's list capacity, whatever a larger workspace would offer this small batch
        B.fcap = std::min<uint32_t>(B.fcap, HVS_FCAP);
        B.gcap = std::min<uint32_t>(B.gcap, HVS_GCAP);
    }
    B.knn = c->k;
    B.topcap = c->k <= 128u ? 128u : 256u;
    // sort workspace shared with the exact engine
    Plan p{};
    p.nq_pad = 256;
    p.nchunks = 1;
    return ensure_batch_workspace(c, nqb, p);
}

// slot layout, position ranges, norms and B fragments of one batch (shared by the MFMA engine and the
// range-based exact engine)
// `count_sn` (filter batches under a mask or a sampled prefix, where hvs_k_prep's own count of whole ranges does not do): the
// batch's passing pairs among ids < *count_sn are counted here, between the layout and hvs_k_prep -- hvs_k_prep empties the
// range of a query that has no usable bound, and that query's pairs count like any other's.
int prep_batch(hvs_ctx* c, uint32_t q0, uint32_t nqb, bool count_pairs, int fmt, bool host_counts = false,
               const uint32_t* list = nullptr, uint32_t want_fcap = HVS_FCAP, const uint32_t* count_sn = nullptr)
{
    int rc = ensure_filter_workspace(c, nqb, want_fcap);
    if (rc) return rc;
    HvsBatch& B = c->fb;
    const uint32_t n = c->n_indexed;  // (positions of the orderings)
    // ~4096 queries of a predicate class per start-position bin (32 groups); inside a bin queries are
    // ordered by range end, so the 4 groups of a filter workgroup stream nearly the same run of tiles.  The class
    // populations stay on the device (hvs_k_query_keys2 reads them there); only the range-scan exact engine, whose
    // launch shapes depend on them, waits for a copy (`host_counts`).
    HVS_HIP(c, hipMemsetAsync(c->d_layout + 8, 0, 8 * sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(hvs_k_count_classes, dim3((nqb + 255u) / 256u), dim3(256), 0, c->stream, c->d_q, q0, nqb, list,
                       c->d_layout + 8);
    if (host_counts) {
        uint32_t counts[5] = {0, 0, 0, 0, 0};
        HVS_HIP(c, hipMemcpyAsync(counts, c->d_layout + 8, sizeof(counts), hipMemcpyDeviceToHost, c->stream));
        HVS_HIP(c, hipStreamSynchronize(c->stream));
        for (int k = 0; k < 5; ++k) c->class_counts[k] = counts[k];
    }
    hipLaunchKernelGGL(hvs_k_query_keys2, dim3((nqb + 255u) / 256u), dim3(256), 0, c->stream, c->d_q, q0, nqb, list, c->ord[0].keys,
                       c->ord[1].keys, n, c->d_layout + 8, c->d_keys, c->d_qidx, c->d_qra, c->d_qrb);
    size_t tmp = c->sort_tmp_bytes;
    HVS_HIP(c, rocprim::radix_sort_pairs(c->d_sort_tmp, tmp, c->d_keys, c->d_keys_sorted, c->d_qidx, c->d_qorder,
                                         (size_t)nqb, 0, 64, c->stream));
    hipLaunchKernelGGL(hvs_k_layout, dim3(std::min(hvs_ceil_div(B.nslots, 1024u), 1024u)), dim3(1024), 0, c->stream, c->d_keys_sorted, c->d_qorder, nqb, B.nslots, q0, list,
                       c->d_qra, c->d_qrb, B.qid, B.rank, B.ra, B.rb, c->d_layout);
    if (count_sn) {
        if (masked(c)) {
            if ((rc = count_masked_pairs(c, *count_sn))) return rc;
        } else {
            hipLaunchKernelGGL(hvs_k_count_prefix_pairs<false>, dim3(B.nslots), dim3(64), 0, c->stream, B, c->ord[0].perm, c->ord[1].perm, *count_sn,
                               c->call.d_counters, c->rs.d_live);
        }
    }
    // (last argument: the batch is for a filter engine -- `host_counts` is the exact engine's range scan, which answers every
    // query itself, non-finite ones included)
    with_capped(c, [&](auto WT) {  // (capped: the slots' thresholds start at the queries' caps)
        hipLaunchKernelGGL(hvs_k_prep<decltype(WT)::value>, dim3(B.ngroups), dim3(4 * HVS_GROUP), 0, c->stream, c->d_q, B, count_pairs ? 1 : 0,
                           c->call.d_counters, fmt, c->d_quant, c->d_bounds, host_counts ? 0 : 1, c->qs.eng.d_max_d2);
    });
    HVS_HIP(c, hipGetLastError());
    return HVS_OK;
}

// The tail of the batch in c->fb (hvs_k_scan_tail): ids [n_indexed, sn), if there are any.  `count`: the batch's pairs go
// to the call's counters (not in re-run batches).
bool have_tail(const hvs_ctx* c, uint32_t sn) { return c->have_order && sn > c->n_indexed; }
void launch_tail(hvs_ctx* c, uint32_t sn, const HvsTailOut& out, bool count)
{
    const HvsBatch& B = c->fb;
    with_order_cap_mask(c, [&](auto ST, auto CAPT, auto MT) {
        with_after(c, [&](auto AT, auto XT) {
            hipLaunchKernelGGL((hvs_k_scan_tail<decltype(ST)::value, decltype(CAPT)::value, decltype(MT)::value, decltype(AT)::value, decltype(XT)::value>),
                               dim3((B.nslots + 255u) / 256u), dim3(256), 0, c->stream, c->d_data, c->d_q, B, out, c->n_indexed, sn, c->call.d_counters,
                               count ? 1 : 0, c->rs.d_live, c->qs.eng.d_after_lo, excl_arg(c));
        });
    });
}

// The stale rows of the batch in c->fb (hvs_k_scan_stale): the prefix of the ascending stale list with id < sn
// (under a mask sn is the cut; stale_below).  0: nothing to launch.
void launch_stale(hvs_ctx* c, uint32_t m, const HvsTailOut& out, bool count)
{
    const HvsBatch& B = c->fb;
    with_order_cap_mask(c, [&](auto ST, auto CAPT, auto MT) {
        with_after(c, [&](auto AT, auto XT) {
            hipLaunchKernelGGL((hvs_k_scan_stale<decltype(ST)::value, decltype(CAPT)::value, decltype(MT)::value, decltype(AT)::value, decltype(XT)::value>),
                               dim3((B.nslots + 255u) / 256u), dim3(256), 0, c->stream, c->d_data, c->d_q, B, out, c->rs.d_stale_ids, m,
                               c->call.d_counters, count ? 1 : 0, c->rs.d_live, c->qs.eng.d_after_lo, excl_arg(c));
        });
    });
}

// Exact engine on top of the index.  Queries with a categorical predicate (types 1 and 3) scan only
// their position range of the (C,T) ordering (hvs_k_scan_ranges): ~1 % / 0.25 % of the rows, 17-25x
// faster than scanning everything.  Type-0 and type-2 queries keep the sequential full scan in original
// row order (hvs_k_scan_exact_lds streams D once, staged through LDS): a position range is a random
// permutation of the rows, and measured on D=1e7 gathering 25 % of them (type 2) is slower than
// streaming all of them (8.2 k vs 14 k queries/s).
int run_batch_exact_ranges(hvs_ctx* c, uint32_t q0, uint32_t nqb, uint32_t sn)
{
    int rc = prep_batch(c, q0, nqb, sn >= c->n_indexed && !masked(c), HVS_FMT_BF16, true);  // (the range scan uses the ranges only)
    if (rc) return rc;
    HvsBatch& B = c->fb;
    const bool tail = have_tail(c, sn);  // rows behind the index: counted for every class, scanned here for the range classes
    const uint32_t stale = stale_below(c, sn);  // likewise the indexed rows whose index entry is stale
    if (masked(c)) {
        if ((rc = count_masked_pairs(c, sn))) return rc;
    } else if (sn < c->n_indexed)
        hipLaunchKernelGGL(hvs_k_count_prefix_pairs<false>, dim3(B.nslots), dim3(64), 0, c->stream, B, c->ord[0].perm, c->ord[1].perm, sn,
                           c->call.d_counters, c->rs.d_live);
    // slot layout of hvs_k_layout: classes 0..3 padded to 32 slots each, then the T-ordering class (type 2)
    // from the next filter-workgroup boundary
    const uint32_t nq0 = c->class_counts[0], nq2 = c->class_counts[4];
    const uint32_t slot_begin = hvs_ceil_div(nq0, 32u) * 32u;
    uint32_t slot_end = slot_begin;
    for (int k = 1; k < 4; ++k) slot_end += hvs_ceil_div(c->class_counts[k], 32u) * 32u;
    const uint32_t slot2 = hvs_ceil_div(slot_end, HVS_WG_WAVES * HVS_GROUP) * (HVS_WG_WAVES * HVS_GROUP);
    if (nq0 && (rc = run_batch_exact(c, 0, nq0, sn, B.qid, false))) return rc;
    if (nq2 && (rc = run_batch_exact(c, 0, nq2, sn, B.qid + slot2, false))) return rc;
    if (slot_begin >= slot_end) {
        // (the full scans above walked the tail and the stale rows themselves: their pairs only)
        if (tail) launch_tail(c, sn, HvsTailOut{nullptr, nullptr, nullptr, 0u, 0u, 0u}, true);
        if (stale) launch_stale(c, stale, HvsTailOut{nullptr, nullptr, nullptr, 0u, 0u, 0u}, true);
        if (tail || stale) HVS_HIP(c, hipGetLastError());
        return HVS_OK;
    }
    const uint32_t waves = (slot_end - slot_begin + 63u) / 64u;
    uint32_t nchunks = std::max(1u, std::min(64u, (8192u + waves - 1u) / waves));
    nchunks = std::min(nchunks, std::max(1u, (1u << 20) / B.nslots));  // candidate lists: at most 2 GB
    // (the tail's keys and the stale rows' keys: one more chunk of lists each -- a list of the exact engine holds c->cap keys,
    // which is what one such scan may fill before it cuts its segment back to k)
    const uint32_t xchunks = (tail ? 1u : 0u) + (stale ? 1u : 0u);
    const size_t lists = (size_t)B.nslots * (nchunks + xchunks);
    if (lists > c->cand_lists) {
        if ((rc = dev_alloc(c, &c->d_cand, lists * (size_t)c->cap))) return rc;
        if ((rc = dev_alloc(c, &c->d_cand_cnt, lists))) return rc;
        c->cand_lists = lists;
    }
    HVS_HIP(c, hipMemsetAsync(c->d_cand_cnt, 0, lists * sizeof(uint32_t), c->stream));
    const int ev = kernel_timer_begin(c);
    const dim3 grid((slot_end + 255u) / 256u, nchunks);
    with_order_cap_mask(c, [&](auto ST, auto CAPT, auto MT) {
        with_capped_after(c, [&](auto WT, auto AT, auto XT) {
            hipLaunchKernelGGL(
                (hvs_k_scan_ranges<decltype(ST)::value, decltype(CAPT)::value, decltype(MT)::value, decltype(WT)::value, decltype(AT)::value, decltype(XT)::value>), grid,
                dim3(256), 0, c->stream, c->d_data, sn, c->d_q, B, c->ord[0].perm, c->ord[1].perm, nchunks, slot_begin, slot_end, c->d_cand,
                c->d_cand_cnt, c->call.d_counters, index_mask(c), c->qs.eng.d_after_lo, excl_arg(c));
        });
    });
    kernel_timer_end(c, ev);
    // (under caps the tail and stale scans admit against the slots' thresholds, which hvs_k_prep set to the caps)
    const float* scan_tau = capped(c) ? B.tau : nullptr;
    if (tail)
        launch_tail(c, sn, HvsTailOut{c->d_cand + (size_t)nchunks * B.nslots * (size_t)c->cap, c->d_cand_cnt + (size_t)nchunks * B.nslots, scan_tau,
                                      (uint32_t)c->cap, slot_begin, slot_end}, true);
    if (stale) {
        const size_t at = (size_t)(nchunks + (tail ? 1u : 0u)) * B.nslots;
        launch_stale(c, stale, HvsTailOut{c->d_cand + at * (size_t)c->cap, c->d_cand_cnt + at, scan_tau, (uint32_t)c->cap, slot_begin, slot_end}, true);
    }
    const uint32_t nsel = slot_end - slot_begin;
    launch_select(c, B.qid + slot_begin, nsel, B.nslots, nchunks + xchunks, c->d_cand + (size_t)slot_begin * (size_t)c->cap,
                  c->d_cand_cnt + slot_begin);
    HVS_HIP(c, hipGetLastError());
    return HVS_OK;
}

// work-item lists of the batch just prepared (all levels at once; see HvsItems in hvs_filter.h)
// buffers of the work-item lists for the batch whose slot layout ensure_filter_workspace has just set (c->fb.ngroups)
int ensure_items(hvs_ctx* c)
{
    const HvsBatch& B = c->fb;
    const HvsLevels L = c->lv;
    const uint32_t nquads = hvs_ceil_div(B.ngroups, HVS_WG_WAVES);
    static const uint32_t kItemsPerSlot = env_u32("HVS_SEG_ITEMS", 8u, 1u, 64u);  // work items per resident workgroup a level should make
    const HvsSegs S = hvs_make_segs(L, nquads, 2u * (uint32_t)c->num_cus, kItemsPerSlot);
    c->segs = S;
    const uint32_t nseg = S.first[L.K + 1];
    if (nquads > (1u << HVS_ITEM_QUAD_BITS)) return fail(c, HVS_EINVAL, "internal: too many query quads for the item code");
    int rc;
    if ((rc = ensure_room(c, &c->d_qlo, c->quads_cap, nquads, &c->d_qhi)) ||
        (rc = ensure_room(c, &c->d_segcnt, c->segs_cap, (size_t)nseg + 1u, &c->d_segoff)))
        return rc;
    if (!c->d_lvloff && (rc = dev_alloc(c, &c->d_lvloff, (size_t)32))) return rc;
    if (!c->d_cursor && (rc = dev_alloc(c, &c->d_cursor, (size_t)16))) return rc;
    const size_t worst = (size_t)nquads * (size_t)(nseg - S.first[1]);  // every quad meets every segment (type 0)
    if ((rc = ensure_room(c, &c->d_items, c->items_cap, worst))) return rc;
    return HVS_OK;
}

int build_items(hvs_ctx* c)
{
    int rc = ensure_items(c);
    if (rc) return rc;
    const HvsBatch& B = c->fb;
    const HvsLevels L = c->lv;
    const uint32_t nquads = hvs_ceil_div(B.ngroups, HVS_WG_WAVES);
    const HvsSegs S = c->segs;
    const uint32_t nseg = S.first[L.K + 1];
    HVS_HIP(c, hipMemsetAsync(c->d_cursor, 0, 16 * sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(hvs_k_quad_ranges, dim3(hvs_ceil_div(nquads, 256u)), dim3(256), 0, c->stream, B, nquads, c->d_qlo, c->d_qhi);
    hipLaunchKernelGGL(hvs_k_item_sweep<false>, dim3(nseg), dim3(256), 0, c->stream, L, S, nquads, c->d_qlo, c->d_qhi, c->d_segcnt,
                       c->d_segoff, c->d_items);
    hipLaunchKernelGGL(hvs_k_item_scan, dim3(1), dim3(1024), 0, c->stream, S, c->d_segcnt, c->d_segoff, c->d_lvloff);
    hipLaunchKernelGGL(hvs_k_item_sweep<true>, dim3(nseg), dim3(256), 0, c->stream, L, S, nquads, c->d_qlo, c->d_qhi, c->d_segcnt,
                       c->d_segoff, c->d_items);
    HVS_HIP(c, hipGetLastError());
    return HVS_OK;
}

// Order statistics of the guessed thresholds (see "Guessed thresholds" at hvs_k_merge).  If the rows seen so far were a
// random sample holding a fraction F of the query's rows, the number X of unseen rows below the sample's m-th smallest
// distance would be negative binomial, P(X = x) = C(x + m - 1, x) F^m (1 - F)^x, and a threshold at that distance leaves
// fewer than k rows below it iff X + m < k.  guess_m: the smallest m with P(X <= k - m - 1) <= target (m = k cannot fail).
uint32_t guess_m(double F, uint32_t k, double target)
{
    if (!(F > 0.0)) return k;
    if (F >= 1.0) return k;  // every row has been seen: only the k-th smallest itself leaves k rows below it
    for (uint32_t m = 1; m < k; ++m) {
        double lp = (double)m * std::log(F), cdf = 0.0;  // log P(X = 0)
        const double l1 = std::log1p(-F);
        for (uint32_t x = 0; x + m < k; ++x) {
            cdf += std::exp(lp);
            lp += std::log((double)(x + m) / (double)(x + 1u)) + l1;
        }
        if (cdf <= target) return m;
    }
    return k;
}
// `proven` (retry batches): m = k at every level -- the proven threshold, which cannot fail (a query that
// failed under a guess did so because the rows it had seen were unlucky, and a larger guess from the same rows shares
// that luck)
HvsGuessTable plan_guess(uint32_t k, bool proven, uint32_t pfail)
{
    HvsGuessTable G{};
    const double target = std::pow(10.0, -(double)pfail);
    for (int i = 0; i < HVS_GUESS_STEPS; ++i)
        G.m[i] = (uint16_t)(proven ? k : guess_m(std::exp2(-(double)i / 8.0), k, target));
    G.floor_m = (uint16_t)std::min(k, proven ? k : kGuessMid);
    G.last_m = (uint16_t)(proven ? k : 0u);
    return G;
}

// candidate keys per slot and round of a batch that runs every level with the PROVEN threshold (retry batches): up to
// k (radix - 1) candidates per query and level, twice that for the band
uint32_t proven_fcap(const hvs_ctx* c)
{
    uint32_t rmax = 2u;
    for (uint32_t j = 1; j <= c->lv.K; ++j) rmax = std::max(rmax, c->lv.radix[j]);
    return std::max<uint32_t>(HVS_FCAP, hvs_ceil_div(2u * c->k * (rmax - 1u), 256u) * 256u);
}
// queries per retry batch: as many as the candidate workspace the call's own batches already allocated can serve with
// proven_fcap keys per slot -- re-running a long list must not ask for 3x the workspace of the batches it came from
uint32_t proven_batch_step(const hvs_ctx* c)
{
    const size_t fit = c->fb_cand_entries / proven_fcap(c);
    const size_t pad = 5u * 32u + (HVS_WG_WAVES + 1u) * HVS_GROUP + HVS_GROUP;  // (slot padding of ensure_filter_workspace)
    uint32_t step = fit > pad + 4096u ? (uint32_t)std::min<size_t>(fit - pad, kBatchMfma) : 4096u;
    step = std::max(512u, step / 512u * 512u);
    return std::min(step, kBatchMfma);
}

// One batch through the filter engine: the resident range [q0, q0 + nqb), or the nqb query indices in the device array
// `list` (retry batches: `proven_last`, failures go to the exact engine); `gates`: of a batch of a call on two lanes (HvsLaneGates).
int run_batch_mfma(hvs_ctx* c, uint32_t q0, uint32_t nqb, uint32_t sn, const uint32_t* list, bool proven_last, BatchGates gates)
{
    const int fmt = c->fmt.built;
    const uint32_t want_fcap = proven_last ? proven_fcap(c) : HVS_FCAP;
    const bool count_in_prep = sn >= c->n_indexed && !list && !masked(c);  // whole ranges: hvs_k_prep counts them as it goes
    int rc = prep_batch(c, q0, nqb, count_in_prep, fmt, false, list, want_fcap, !list && !count_in_prep ? &sn : nullptr);
    if (rc) return rc;
    if ((rc = build_items(c))) return rc;
    HvsBatch& B = c->fb;
    const HvsLevels L = c->lv;
    HvsItems W{c->d_items, c->d_lvloff, c->d_cursor, HVS_SEG};
    const uint32_t n = c->n_indexed;  // positions of the orderings; the padding of the final merge counts from the end of D (c->n)
    if (c->guess_k != c->k) {  // (tables are made on first use: 168 x ~100 negative-binomial sums each, ~10 ms on the host)
        for (bool& h : c->guess_have) h = false;
        c->guess_k = c->k;
    }
    const uint32_t gslot = proven_last ? 0u : (c->force_pfail ? c->force_pfail : guess_pfail_for(nqb));  // slot 0: the proven table
    if (!c->guess_have[gslot]) {
        c->guess_tab[gslot] = plan_guess(c->k, proven_last, gslot ? gslot : 3u);
        c->guess_have[gslot] = true;
    }
    const HvsGuessTable G = c->guess_tab[gslot];
    B.fail_code = proven_last ? HVS_FAIL_EXACT : HVS_FAIL_RETRY;

    if (gates.wait_heavy) HVS_HIP(c, hipStreamWaitEvent(c->stream, gates.wait_heavy, 0));  // (two lanes: see HvsLaneGates::ev_pdone)
    // level 0 by the exact kernel; small batches cut it into chunks so that enough waves are in flight
    const uint32_t l0blocks = L.off[1] - L.off[0];
    const uint32_t seed_waves = hvs_ceil_div(B.nslots, 64u);
    uint32_t seed_chunks = 1u;
    if (l0blocks <= B.fcap / 32u && seed_waves < kSeedWaves) seed_chunks = std::min(l0blocks, hvs_ceil_div(kSeedWaves, seed_waves));
    with_cap_mask(c, [&](auto CAPT, auto MT) {
        with_capped_after(c, [&](auto WT, auto AT, auto XT) {
            hipLaunchKernelGGL((hvs_k_seed_exact<decltype(CAPT)::value, decltype(MT)::value, decltype(WT)::value, decltype(AT)::value, decltype(XT)::value>),
                               dim3((B.nslots + 255u) / 256u, std::max(1u, seed_chunks)), dim3(256), 0, c->stream, c->d_data, n, sn, c->d_q, B,
                               c->ord[0].perm, c->ord[1].perm, c->ord[0].bpos, c->ord[1].bpos, L, c->call.d_counters, std::max(1u, seed_chunks),
                               index_mask(c), c->qs.eng.d_after_lo, excl_arg(c));
        });
    });
    // merge behind a level: top-k, and the threshold of level `next` (its order statistic from the guess plan)
    auto launch_merge = [&](bool final, uint32_t next) {
        with_cap_mask(c, [&](auto CAPT, auto MT) {
            constexpr int CAP = decltype(CAPT)::value;
            if (final)  // (only the final merge pads and drops keys beyond a cap: the merges in front of it have no masked or capped form)
                with_capped_after(c, [&](auto WT, auto AT, auto XT) {
                    hipLaunchKernelGGL((hvs_k_merge<true, CAP, decltype(MT)::value, decltype(WT)::value, decltype(AT)::value, decltype(XT)::value>),
                                       dim3((B.nslots + 3u) / 4u), dim3(256), 0, c->stream, c->d_data, c->n, c->d_q, B, c->d_bounds,
                                       c->padding ? 1 : 0, c->d_out_ids, c->d_out_dists, fmt, c->d_quant, L, next, G, c->rs.d_pad_ids, c->qs.eng.d_max_d2,
                                       c->call.d_counters, c->qs.eng.d_after_lo, excl_arg(c));
                });
            else
                hipLaunchKernelGGL((hvs_k_merge<false, CAP, false>), dim3((B.nslots + 3u) / 4u), dim3(256), 0, c->stream, c->d_data, c->n, c->d_q, B,
                                   c->d_bounds, c->padding ? 1 : 0, c->d_out_ids, c->d_out_dists, fmt, c->d_quant, L, next, G, c->rs.d_pad_ids,
                                   c->qs.eng.d_max_d2, c->call.d_counters, c->qs.eng.d_after_lo, HvsExcl{});
        });
    };
    // Rows behind the index: scanned exactly once per batch, in front of the final merge, into the lists the
    // last re-scoring filled -- every tail row with distance <= tau_last is then held beside every indexed one, which is all
    // the final check needs.  The guessed thresholds never see these rows.
    // Likewise, right behind them, the indexed rows whose index entry is stale: no list holds one of them so far.
    auto tail_before_final = [&]() {
        if (have_tail(c, sn)) launch_tail(c, sn, HvsTailOut{B.cand, B.candcnt, B.tau, B.fcap, 0u, B.nslots}, !list);
        if (const uint32_t m = stale_below(c, sn)) launch_stale(c, m, HvsTailOut{B.cand, B.candcnt, B.tau, B.fcap, 0u, B.nslots}, !list);
    };
    if (L.K == 0u) tail_before_final();
    launch_merge(L.K == 0u, 1u);
    // re-scoring blocks per group: each block stages the group's 128 queries in LDS first, so large batches use
    // few long-lived blocks per group (2: -4 % of the step at 262144 queries) and small batches enough blocks to
    // fill the chip
    const uint32_t rescore_blocks = kRescoreBlocks ? kRescoreBlocks : std::max(2u, std::min(8u, hvs_ceil_div(4096u, B.ngroups)));
    // One filter -> re-score -> merge round per level.  (Sharing a round between the two low levels of a small batch --
    // BASELINE configs[1]/[2], 10^4 queries: m (R - 1) = 1000 rows per query to the exact kernel instead of 2 x 60 for one
    // re-score + merge less -- was measured in round 3: 2.85 ms instead of 2.08 ms per 10^4 mixed queries.  Round 2 measured
    // the same for doubling levels.)
    const HvsFilterKernel filter_kernel = hvs_host_fmt(fmt, c->fmt.i8_rot).filter;  // picked once per batch
    for (uint32_t level = 1; level <= L.K;) {
        const uint32_t last = level;
        // (the groups' entry counters are zero here: hvs_k_prep clears them for the first level, every merge for the next)
        for (; level <= last; ++level) {
            const int ev = kernel_timer_begin(c);
            // a fixed crew of workgroups pulls the level's work items (two resident per CU + spares)
            static const uint32_t kWgsPerCu = env_u32("HVS_FILTER_WGS_PER_CU", 4u, 1u, 16u);
            const dim3 fgrid(kWgsPerCu * (uint32_t)c->num_cus);
            W.segsize = c->segs.seg[level];
            hipLaunchKernelGGL(filter_kernel, fgrid, dim3(64 * HVS_WG_WAVES), 0, c->stream, c->ord[0].tiles, c->ord[1].tiles, c->ord[0].nrm,
                               c->ord[1].nrm, c->ord[0].bpos, c->ord[1].bpos, L, level, B, W, c->call.d_counters);
            kernel_timer_end(c, ev);
            if (level == L.K && gates.record_fdone) HVS_HIP(c, hipEventRecord(gates.record_fdone, c->stream));
            if (level + 1u == L.K && gates.record_pdone) HVS_HIP(c, hipEventRecord(gates.record_pdone, c->stream));
        }
        with_cap_mask(c, [&](auto, auto MT) {
            with_after(c, [&](auto AT, auto XT) {
                constexpr bool M = decltype(MT)::value;
                // (while rows are stale the front end gets both masks and tells stale from dead: HVS_RESCORE_TWO_MASKS)
                const uint32_t nn = c->rs.h_stale.empty() ? n : (n | HVS_RESCORE_TWO_MASKS);
                if constexpr (decltype(XT)::value) {
                    const auto rescore = fmt == HVS_FMT_I8X16 ? hvs_k_rescore<true, M, const uint64_t*, HvsExcl> : hvs_k_rescore<false, M, const uint64_t*, HvsExcl>;
                    hipLaunchKernelGGL(rescore, dim3(rescore_blocks, B.ngroups), dim3(64 * HVS_RESCORE_WAVES), 0, c->stream, c->d_data, nn, sn,
                                       c->d_q, B, c->ord[0].perm, c->ord[1].perm, c->call.d_counters, index_mask(c),
                                       static_cast<const uint64_t*>(c->qs.eng.d_after_lo), excl_arg(c));
                } else if constexpr (decltype(AT)::value) {
                    const auto rescore = fmt == HVS_FMT_I8X16 ? hvs_k_rescore<true, M, const uint64_t*> : hvs_k_rescore<false, M, const uint64_t*>;  // (entry format)
                    hipLaunchKernelGGL(rescore, dim3(rescore_blocks, B.ngroups), dim3(64 * HVS_RESCORE_WAVES), 0, c->stream, c->d_data, nn, sn,
                                       c->d_q, B, c->ord[0].perm, c->ord[1].perm, c->call.d_counters, index_mask(c),
                                       static_cast<const uint64_t*>(c->qs.eng.d_after_lo));
                } else {
                    const auto rescore = fmt == HVS_FMT_I8X16 ? hvs_k_rescore<true, M> : hvs_k_rescore<false, M>;
                    hipLaunchKernelGGL(rescore, dim3(rescore_blocks, B.ngroups), dim3(64 * HVS_RESCORE_WAVES), 0, c->stream, c->d_data, nn, sn,
                                       c->d_q, B, c->ord[0].perm, c->ord[1].perm, c->call.d_counters, index_mask(c));
                }
            });
        });
        if (last == L.K) tail_before_final();
        launch_merge(last == L.K, last + 1u);
    }
    // queries this batch could not answer go on the call's lists (retry with a proven threshold / exact engine); they
    // are answered again when the call's results are first needed (resolve_overflow) -- the batch never waits for the host
    hipLaunchKernelGGL(hvs_k_collect_overflow, dim3((B.nslots + 255u) / 256u), dim3(256), 0, c->stream, B, c->call.d_ovf_list,
                       c->call.d_ovf_count, c->call.d_retry_list, c->call.d_ovf_count + 1);
    HVS_HIP(c, hipGetLastError());
    return HVS_OK;
}

// Queries the call's batches could not answer.  First the retry list (a guessed threshold that failed its check, or a list
// that overflowed under it): filter batches whose last level uses the proven threshold; what fails there joins the
// exact list.  Then the exact engine re-runs the exact list (rare: thousands of equal distances, queries far outside the
// data's bounding box, non-finite components).  Called wherever a call's results or timing leave the library; costs
// one stream synchronisation per call (two more when there is something to re-run).
int resolve_overflow(hvs_ctx* c)
{
    if (!c->call.pending) return HVS_OK;
    HVS_HIP(c, hipSetDevice(c->device));
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    c->call.pending = false;
    uint32_t novf = c->call.h_ovf[0];
    const uint32_t nretry = c->call.h_ovf[1];
    if (novf == 0u && nretry == 0u) return HVS_OK;
    // A list through filter batches with proven thresholds, then the exact list's new length.  *done: the queries that got a
    // batch -- what is left when one cannot get its workspace is appended to the exact engine's list, which needs none.
    auto rerun_proven = [&](const uint32_t* list, uint32_t count, uint32_t* done) -> int {
        const uint32_t step = proven_batch_step(c);
        for (*done = 0; *done < count; *done += std::min(step, count - *done)) {
            int rc = run_batch_mfma(c, 0, std::min(step, count - *done), c->call.pend_sn, list + *done, true);
            if (rc == HVS_ENOMEM) {
                (void)hipGetLastError();
                uint32_t have = 0;
                if ((rc = fetch_fail_counts(c, &have))) return rc;
                const uint32_t rest = count - *done, total = have + rest;
                HVS_HIP(c, hipMemcpyAsync(c->call.d_ovf_list + have, list + *done, (size_t)rest * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
                HVS_HIP(c, hipMemcpyAsync(c->call.d_ovf_count, &total, sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
                HVS_HIP(c, hipStreamSynchronize(c->stream));
                c->err.clear();
                break;
            }
            if (rc) return rc;
        }
        return fetch_fail_counts(c, &novf);
    };
    if (nretry) {
        uint32_t done = 0;
        c->call.timing.retry_queries = nretry;
        if (int rc = rerun_proven(c->call.d_retry_list, nretry, &done)) return rc;
    }
    // Many queries without a usable INT8 bound in one call (the planner's probe uses rows of D as queries: real queries can
    // lie far outside the data's box, where the clip term drowns the band): under HVS_ENGINE_AUTO the 16-bit float tiles
    // are built now -- for this call's list and for the calls to come -- instead of sending them all to the exact engine
    // at 1 % of a filter's rate.  The list moves aside (the filter batches append their own failures to the exact list).
    if (c->engine == HVS_ENGINE_AUTO && HVS_IS_I8(c->fmt.built) && novf >= std::max(256u, c->call.timing.nq / 50u) &&
        env_u32("HVS_DEMOTE", 1u, 0u, 1u)) {
        if (c->call.demote_cap < c->res_cap) {
            int rc = dev_alloc(c, &c->call.d_demote_list, (size_t)c->res_cap);
            if (rc) return rc;
            c->call.demote_cap = c->res_cap;
        }
        // The 16-bit float tiles first: when HBM has no room for them next to D (they are 1.7x the INT8 tiles) the INT8
        // tiles come back and the exact engine answers the list as it always did -- slower, never an error.
        const int had = c->fmt.built;
        int rc = build_tiles_chain(c, next_format_down(c, had));
        if (rc == HVS_ENOMEM || (!rc && c->fmt.built == HVS_FMT_NONE)) {
            (void)hipGetLastError();
            c->err.clear();
            rc = build_tiles_chain(c, had);
            if (rc == HVS_ENOMEM) {
                (void)hipGetLastError();
                c->err.clear();
                rc = HVS_OK;
            }
            if (rc) return rc;
        } else if (rc) {
            return rc;
        } else {
            HVS_HIP(c, hipMemcpyAsync(c->call.d_demote_list, c->call.d_ovf_list, (size_t)novf * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
            HVS_HIP(c, hipMemsetAsync(c->call.d_ovf_count, 0, sizeof(uint32_t), c->stream));
            c->fmt.planned = c->fmt.built;
            if ((rc = rerun_proven(c->call.d_demote_list, novf, &c->call.demoted_queries))) return rc;
            c->call.timing.flags |= HVS_TIMING_FORMAT_CHANGED;
            c->call.timing.engine = timing_engine_for(c->fmt.built);
        }
    }
    c->call.timing.fallback_queries = novf;
    for (uint32_t off = 0; off < novf; off += kBatch) {
        const uint32_t m = std::min(kBatch, novf - off);
        int rc = run_batch_exact(c, 0, m, c->call.pend_sn, c->call.d_ovf_list + off, false, false);
        if (rc) return rc;
    }
    HVS_HIP(c, hipEventRecord(c->call.ev_q1, c->stream));  // the re-runs belong to the call's device time
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    return HVS_OK;
}

// Host copy between pageable and pinned memory.  One thread moves ~10 GB/s; the first batch's queries and the last
// batch's results of a call sit on the critical path (nothing computes under them), so pieces of 4 MB and more are cut
// over up to 4 threads.
void staging_copy(void* dst, const void* src, size_t bytes)
{
    static const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    static const unsigned kMaxParts = env_u32("HVS_STAGE_THREADS", 8u, 1u, 64u);  // (4 until round 4: ~15 GB/s; 8: ~25 GB/s on the GPU boxes' hosts)
    const unsigned parts = bytes >= (4u << 20) ? std::min(kMaxParts, std::max(1u, hw / 4u)) : 1u;
    if (parts <= 1u) {
        std::memcpy(dst, src, bytes);
        return;
    }
    const size_t chunk = ((bytes / parts) + 4095u) & ~(size_t)4095u;
    std::vector<std::thread> th;
    th.reserve(parts - 1u);
    for (unsigned p = 1; p < parts; ++p) {
        const size_t off = (size_t)p * chunk;
        if (off >= bytes) break;
        const size_t len = std::min(chunk, bytes - off);
        th.emplace_back([=]() { std::memcpy(static_cast<char*>(dst) + off, static_cast<const char*>(src) + off, len); });
    }
    std::memcpy(dst, src, std::min(chunk, bytes));
    for (auto& t : th) t.join();
}

// Batch schedule of one call (sizes in queries, in order).  Resident runs and the exact engines cut the call into
// full batches.  `host_pipeline` (hvs_query): the first batch's queries and the last batch's results are the only
// transfers the pipeline cannot hide, so those two batches are small (kBatchMfma / 8) once the call is large enough to
// pay for two extra batches, and the batches between share the rest evenly in whole quads of 512 queries.
// The host pipeline of hvs_query stages its input by THIS schedule (the hooks receive the sizes), never by a guess of it.
std::vector<uint32_t> batch_schedule(uint32_t nq, uint32_t step, bool ramp_allowed)
{
    std::vector<uint32_t> out;
    // (calls below 2^20 queries -- e.g. one GPU's share of BASELINE configs[3] on an 8-GPU node, 5 x 10^5 -- stay ONE batch:
    // with the staging copies cut over 4 threads the two exposed transfers cost ~9 ms, less than what two small edge
    // batches lose in efficiency; measured in round 3, 5 x 10^5 queries host -> host: one batch 178.5 ms, ramped 185.1 ms,
    // two / three equal batches 183.3 / 189.0 ms, resident 169 ms)
    const uint32_t edge = kBatchMfma / 8u;
    const bool ramp = ramp_allowed && edge >= 1024u && nq >= 4u * edge;
    if (!ramp) {
        for (uint32_t off = 0; off < nq; off += step) out.push_back(std::min(step, nq - off));
        return out;
    }
    out.push_back(edge);
    uint32_t middle_left = nq - 2u * edge;
    uint32_t middle_batches = hvs_ceil_div(middle_left, step);
    while (middle_left) {
        const uint32_t nqb = std::min(middle_left, hvs_ceil_div(hvs_ceil_div(middle_left, middle_batches), 512u) * 512u);
        out.push_back(nqb);
        middle_left -= nqb;
        middle_batches -= 1u;
    }
    out.push_back(edge);
    return out;
}

// The sampled prefix of one call: `sn` is what every kernel's sampled-prefix test compares ids against, `sampled` of `of_rows`
// rows are searched (live ones under a mask).  The public entry points derive it from the caller's sample_proportion
// (cut_for); a part of a row-partitioned context is handed its share of the whole data set's prefix as a row count
// (cut_rows): no fraction expresses a cut inside a part.
struct RowCut {
    uint32_t sn, sampled, of_rows;
};
RowCut cut_rows(const hvs_ctx* c, uint32_t rows) { return RowCut{rows, rows, c->n}; }
RowCut cut_for(hvs_ctx* c, float sample_proportion)
{
    uint32_t sn = sample_rows(sample_proportion, c->n);
    uint32_t sampled = sn, of_rows = c->n;
    if (c->rs.n_dead) {
        // live-row mask: the rows searched are the first sn_live live rows = "id < cut and live" (hvs_mask_plan); `sn` is the
        // cut id from here on -- what every kernel's sampled-prefix test compares against
        if (!c->rs.cut_valid || std::memcmp(&c->rs.cut_sp, &sample_proportion, sizeof(float)) != 0) {
            uint32_t n_live = 0;
            hvs_mask_plan(c->rs.h_live.data(), c->n, c->k, sample_proportion, &n_live, &c->rs.cut_id, nullptr);
            c->rs.cut_sn_live = sample_rows(sample_proportion, n_live);
            c->rs.cut_sp = sample_proportion;
            c->rs.cut_valid = true;
        }
        of_rows = c->n - c->rs.n_dead;
        sampled = c->rs.cut_sn_live;
        sn = sampled ? c->rs.cut_id : 0u;
    }
    return RowCut{sn, sampled, of_rows};
}

// The spare lane's workspace for batches of up to nqb queries, with the spare lane swapped in (the caller's LaneGuard).  Without room
// for it: HVS_OK and gates.lanes_failed.  (HVS_TEST_NO_SPARE=1: tests take the out-of-memory path without filling 288 GB)
int ensure_spare_lane(hvs_ctx* c, uint32_t nqb)
{
    static const bool kTestNoSpare = env_u32("HVS_TEST_NO_SPARE", 0u, 0u, 1u) != 0u;
    int rc = kTestNoSpare ? HVS_ENOMEM : ensure_filter_workspace(c, nqb);
    if (!rc) rc = ensure_items(c);
    if (rc != HVS_ENOMEM) return rc;
    (void)hipGetLastError();
    c->err.clear();
    c->gates.lanes_failed = true;
    return HVS_OK;
}

// Resident queries [q0, q0 + nq) while candidate lists are attached: one launch of hvs_k_scan_candidates, a wave per
// query, straight into the result rows.  No engine, no index, no tile format and no re-run is involved: hvs_set_engine has no
// effect on such a call.  It leaves behind what a call leaves behind.
template <typename Hooks>
int run_candidates(hvs_ctx* c, uint32_t q0, uint32_t nq, RowCut cut, Hooks&& hooks)
{
    HvsQuerySet& s = c->qs;
    s.call_capped = capped(c);
    s.call_after = has_after(c);
    s.excl.call = has_excl(c);
    s.call_rset = has_rset(c);
    s.cand.call = true;
    s.in.call = false;
    s.answered(q0, nq, c->k, s.set_gen);
    int rc = call_begin(c);
    if (rc) return rc;
    if ((rc = hooks.before(0u, nq))) return rc;
    if (nq) {
        const int ev = kernel_timer_begin(c);
        const HvsExcl cand{s.cand_at.d_begin, s.cand_at.d_count, s.cand.d_ids};
        HvsExcl excl = excl_arg(c);  // (the scan tells "no lists" by a null `begin`; the sets ride along either way)
        if (!has_excl(c)) excl.begin = excl.count = excl.ids = nullptr;
        with_cap(c->k <= 128u ? 256 : 512, [&](auto CAPT) {
            auto launch = [&](auto ST) {
                hipLaunchKernelGGL((hvs_k_scan_candidates<decltype(ST)::value, decltype(CAPT)::value>), dim3((nq + 3u) / 4u), dim3(256), 0, c->stream,
                                   c->d_data, c->n, cut.sampled ? cut.sn : 0u, c->d_q, q0, nq, cand, masked(c) ? c->rs.d_live : nullptr,
                                   capped(c) ? c->qs.eng.d_max_d2 : nullptr, has_after(c) ? c->qs.eng.d_after_lo : nullptr, excl, c->padding ? 1 : 0,
                                   masked(c) ? c->rs.d_pad_ids : nullptr, c->d_out_ids, c->d_out_dists, c->k, c->call.d_counters);
            };
            if (c->scalar_order)
                launch(std::true_type{});
            else
                launch(std::false_type{});
        });
        kernel_timer_end(c, ev);
        HVS_HIP(c, hipGetLastError());
    }
    if ((rc = hooks.after(0u, nq, 0u))) return rc;
    return call_enqueued(c, nq, false, cut.sn);
}

// Hooks of run_queries: `before(off, nqb)` is called before the kernels of a batch are enqueued (hvs_query makes the
// compute stream wait for the batch's queries there: a batch never starts before its input is on the device);
// `after(off, nqb, next_nqb)` after they have been enqueued (the host pipeline of hvs_query hangs its copies there);
// queries [q0 + off, q0 + off + nqb) are complete on the stream at that point, except for overflowed ones
// (resolve_overflow).
template <typename Hooks>
int run_queries_cut(hvs_ctx* c, uint32_t q0, uint32_t nq, RowCut cut, Hooks&& hooks, bool host_pipeline = false)
{
    if (!c->d_data) return fail(c, HVS_ESTATE, "no data set loaded (hvs_load_data / hvs_gen_data)");
    if ((uint64_t)q0 + nq > c->nq) return fail(c, HVS_EINVAL, "query range outside the resident query set");
    HVS_HIP(c, hipSetDevice(c->device));
    if (int rc = resolve_overflow(c)) return rc;  // an earlier call whose results were never fetched
    if (has_cand(c)) return run_candidates(c, q0, nq, cut, hooks);
    c->qs.cand.call = false;
    const uint32_t sn = cut.sn, sampled = cut.sampled, of_rows = cut.of_rows;
    // The index orders ALL rows: with a sampled prefix [0,sn) the filter still proposes rows >= sn and the
    // exact stages drop them, so its candidate lists grow by n/sn -- used down to sn = n/4, below that
    // the exact engine answers.
    bool mfma = c->have_order && sampled >= of_rows / 4u && sampled > 0u && !c->scalar_order && filter_engine_selected(c);
    if (mfma) {
        // the tiles exist in one format at a time: an engine choice made after the load rebuilds them
        const int want = want_format(c);
        if (want != c->fmt.built) {
            int rc = build_tiles_chain(c, want);
            if (rc) return rc;
        }
        mfma = c->fmt.built != HVS_FMT_NONE;  // (no usable bound at all: the exact engine answers, on the orderings)
    }
    c->qs.call_capped = capped(c);
    c->qs.call_after = has_after(c);
    c->qs.excl.call = has_excl(c);
    c->qs.call_rset = has_rset(c);
    c->qs.in.call = false;  // (in_run sets it once the merge is enqueued)
    c->qs.answered(q0, nq, c->k, c->qs.set_gen);
    if (int rc = call_begin(c)) return rc;
    const bool ranges = !mfma && c->have_order;  // exact engine: scan position ranges when the orderings exist
    const std::vector<uint32_t> sched = batch_schedule(nq, mfma ? kBatchMfma : kBatch, host_pipeline && mfma);
    // Two lanes (HvsLane): every other batch of a filter-engine call runs on the spare lane's stream and workspace, so that
    // its preparation, seed and low levels share the chip with the previous batch's last re-scoring and final merge.  The
    // spare lane starts behind the call's counter resets (ev_q0) and the main stream joins it before the call ends.
    bool two_lanes = mfma && kLanes && sched.size() >= 2 && !c->gates.lanes_failed;
    bool spare_used = false;
    struct JoinOnError {  // a call that fails half-way leaves no kernels running on the spare lane behind the caller's back
        hvs_ctx* c;
        const bool* used;
        bool ok = false;
        ~JoinOnError()
        {
            if (!ok && *used && c->spare.stream) (void)hipStreamSynchronize(c->spare.stream);
        }
    } join_on_error{c, &spare_used};
    uint32_t off = 0;
    for (size_t b = 0; b < sched.size(); ++b) {
        const uint32_t nqb = sched[b];
        LaneGuard lane{c, false};
        if (two_lanes && (b & 1u)) {
            swap_lanes(c);
            lane.on = true;
            // the spare workspace is allocated here, ahead of the batch: without room for it the call stays on one lane
            if (int rcw = ensure_spare_lane(c, nqb)) return rcw;
            if (c->gates.lanes_failed) {
                swap_lanes(c);
                lane.on = false;
                two_lanes = false;
            } else if (!spare_used) {
                HVS_HIP(c, hipStreamWaitEvent(c->stream, c->call.ev_q0, 0));
                spare_used = true;
            }
        }
        // two lanes: preparation behind the previous batch's (other lane) second-to-last filter launch, seed behind its last one
        const bool have_prev = two_lanes && b > 0 && c->lv.K >= 1u;
        if (have_prev) HVS_HIP(c, hipStreamWaitEvent(c->stream, c->gates.start_of(b, c->lv.K), 0));
        int rc = hooks.before(off, nqb);
        if (!rc)
            rc = mfma ? run_batch_mfma(c, q0 + off, nqb, sn, nullptr, false, two_lanes ? c->gates.of_batch(b, have_prev) : BatchGates{})
                      : (ranges ? run_batch_exact_ranges(c, q0 + off, nqb, sn) : run_batch_exact(c, q0 + off, nqb, sn));
        if (rc) return rc;
        if ((rc = hooks.after(off, nqb, b + 1 < sched.size() ? sched[b + 1] : 0u))) return rc;
        if (lane.on) HVS_HIP(c, hipEventRecord(c->gates.ev_lane, c->stream));
        off += nqb;
    }
    if (spare_used) HVS_HIP(c, hipStreamWaitEvent(c->stream, c->gates.ev_lane, 0));
    const int rc = call_enqueued(c, nq, mfma, sn);
    join_on_error.ok = rc == HVS_OK;
    return rc;
}

template <typename Hooks>
int run_queries(hvs_ctx* c, uint32_t q0, uint32_t nq, float sample_proportion, Hooks&& hooks, bool host_pipeline = false)
{
    return run_queries_cut(c, q0, nq, cut_for(c, sample_proportion), hooks, host_pipeline);
}

// ---------------------------------------------------------------------------------------------
// leaf (one GPU) implementations of the C ABI; the multi-GPU root dispatches to them
// ---------------------------------------------------------------------------------------------
struct NoHook {
    int before(uint32_t, uint32_t) const { return HVS_OK; }
    int after(uint32_t, uint32_t, uint32_t) const { return HVS_OK; }
};

int leaf_create(hvs_ctx** out, int device)
{
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0) {
        g_global_err = std::string("hvs_create: no HIP device available (") + hipGetErrorString(e) +
                       "); this library has no CPU fallback";
        return HVS_EHIP;
    }
    if (device < 0) {
        if (hipGetDevice(&device) != hipSuccess) device = 0;
    }
    if (device >= count) {
        g_global_err = "hvs_create: device index out of range";
        return HVS_EINVAL;
    }
    hvs_ctx* c = new (std::nothrow) hvs_ctx();
    if (!c) {
        g_global_err = "hvs_create: out of host memory";
        return HVS_ENOMEM;
    }
    c->device = device;
    auto bail = [&](const char* what, hipError_t err) {
        g_global_err = std::string("hvs_create: ") + what + ": " + hipGetErrorString(err);
        hvs_destroy(c);
        return HVS_EHIP;
    };
    if ((e = hipSetDevice(device)) != hipSuccess) return bail("hipSetDevice", e);
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) c->num_cus = cus;
    }
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) return bail("hipStreamCreate", e);
    if ((e = hipStreamCreateWithFlags(&c->spare.stream, hipStreamNonBlocking)) != hipSuccess) return bail("hipStreamCreate", e);
    if ((e = c->gates.create()) != hipSuccess) return bail("hipEventCreate", e);
    if ((e = hipEventCreate(&c->call.ev_q0)) != hipSuccess) return bail("hipEventCreate", e);
    if ((e = hipEventCreate(&c->call.ev_q1)) != hipSuccess) return bail("hipEventCreate", e);
    if (const char* what = c->pipe.create(c, &e)) return bail(what, e);
    if ((e = hipMalloc(reinterpret_cast<void**>(&c->call.d_counters), HVS_CNT_COUNT * sizeof(unsigned long long))) != hipSuccess)
        return bail("hipMalloc", e);
    if ((e = hipMalloc(reinterpret_cast<void**>(&c->call.d_ovf_count), 2 * sizeof(uint32_t))) != hipSuccess) return bail("hipMalloc", e);
    if ((e = hipMalloc(reinterpret_cast<void**>(&c->d_layout), 16 * sizeof(uint32_t))) != hipSuccess) return bail("hipMalloc", e);
    if ((e = hipHostMalloc(reinterpret_cast<void**>(&c->call.h_ovf), 2 * sizeof(uint32_t), hipHostMallocDefault)) != hipSuccess)
        return bail("hipHostMalloc", e);
    c->call.h_ovf[0] = c->call.h_ovf[1] = 0u;
    c->pipe.warm_streams(c->stream, c->spare.stream, c->call.d_ovf_count, c->call.h_ovf);
    *out = c;
    return HVS_OK;
}

void leaf_destroy(hvs_ctx* c)
{
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    c->pipe.sync();
    if (c->spare.stream) (void)hipStreamSynchronize(c->spare.stream);
    free_index(c);  // (keeps ord[].lp: freed here)
    void* ptrs[] = {c->d_data, c->d_q, c->d_out_ids, c->d_out_dists, c->call.d_counters, c->d_bounds, c->d_quant,
                    c->call.d_ovf_list, c->call.d_ovf_count, c->call.d_retry_list, c->call.d_demote_list, c->ord[0].lp, c->ord[1].lp};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    c->rs.free_device();
    c->qs.free_device();
    c->ord[0].lp = c->ord[1].lp = nullptr;
    {
        HvsPart& P = c->part;
        HvsRowSet::drop(P.d_tail, P.d_gx_ids, P.d_m_ids, P.d_gx_dists, P.d_m_dists, P.d_padded);
        for (hipEvent_t ev : {P.ev_x0, P.ev_x1, P.ev_m1})
            if (ev) (void)hipEventDestroy(ev);
    }
    free_lane(c->spare);
    free_lane(static_cast<HvsLane&>(*c));
    c->gates.destroy();
    if (c->call.h_ovf) (void)hipHostFree(c->call.h_ovf);
    if (c->call.ev_q0) (void)hipEventDestroy(c->call.ev_q0);
    if (c->call.ev_q1) (void)hipEventDestroy(c->call.ev_q1);
    for (hipEvent_t e : c->call.ev_k) (void)hipEventDestroy(e);
    c->pipe.destroy();
}

int attach_for_call(hvs_ctx* c, const float* max_d2, const float* after_d, const uint32_t* after_i, uint32_t nq, const uint32_t* ex_off = nullptr,
                    const uint32_t* ex_ids = nullptr);

// query / result buffers and the batch workspace for calls of up to nq queries (hvs_reserve, hvs_query): keeps the
// ~34 GB of per-batch state of a 2^21-query batch out of the first query's own time
int leaf_reserve(hvs_ctx* c, uint32_t nq)
{
    HVS_HIP(c, hipSetDevice(c->device));
    if (c->qs.in.active) {  // category sets: the engines answer the sub-queries of the first nq queries (one each beyond the resident ones)
        const uint32_t in_set = std::min(nq, c->qs.in.nuq);
        nq = (uint32_t)std::min<uint64_t>((uint64_t)c->qs.in.h_sub_off[in_set] + (nq - in_set), 0xFFFFFFFFull);
    }
    c->reserve_nq = std::max(c->reserve_nq, nq);
    if (nq == 0u) return HVS_OK;
    int rc = ensure_queries(c, nq);
    if (rc) return rc;
    // pinned staging of the host path (ids only: the distance slots follow the first call that asks for distances)
    if ((rc = c->pipe.size_for(c->k, false, nq, nq))) return rc;
    if (c->nq == 0u) c->pipe.warm_dma(c->d_out_ids, c->d_q, (size_t)nq * c->k * sizeof(uint32_t));  // (no resident queries to overwrite)
    // (the filter workspace only when a filter engine is going to run: 4096 <= n < 32768 under AUTO has an index for the
    // range scans of the exact engine, whose batches are kBatch queries)
    if (c->have_order && filter_engine_selected(c)) {
        if ((rc = ensure_filter_workspace(c, std::min(nq, kBatchMfma)))) return rc;
        if ((rc = ensure_items(c))) return rc;
        // calls of two batches and more alternate between two lanes: the spare lane's largest batch under either schedule (the
        // resident API's full batches, hvs_query's ramped ones -- a call of 2 x 10^6 queries is ONE batch resident and three from
        // host memory).  Without this the first such call allocated ~38 GB inside its own time (2.7 s on a 4 x 10^6-query call
        // over two virtual ranks).
        uint32_t spare_nq = 0;
        for (int host = 0; host < 2; ++host) {
            const std::vector<uint32_t> sched = batch_schedule(nq, kBatchMfma, host != 0);
            for (size_t b = 1; b < sched.size(); b += 2) spare_nq = std::max(spare_nq, sched[b]);
        }
        if (kLanes && spare_nq && !c->gates.lanes_failed) {
            LaneGuard lane{c, true};
            swap_lanes(c);
            rc = ensure_spare_lane(c, spare_nq);
        }
        return rc;
    }
    if (c->have_order) return ensure_filter_workspace(c, std::min(nq, kBatch));
    const uint32_t nqb = std::min(nq, kBatch);
    return ensure_batch_workspace(c, nqb, make_plan(nqb, c->n ? c->n : 1u));
}

// ---- row-set state (HvsRowSet): what every call that changes it shares ----
// Every call that changes the rows, the mask, the index or k starts here: an earlier call's pending re-runs belong to the rows,
// the mask and the ids they were asked under, so they run first; then nothing on the device reads what is about to change.
int begin_mutation(hvs_ctx* c)
{
    HVS_HIP(c, hipSetDevice(c->device));
    int rc = resolve_overflow(c);
    if (rc) return rc;
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    return HVS_OK;
}

// Room for `want` elements in *buf with its first `keep` elements preserved.  The new buffer is allocated before the old one
// is released, so a failure leaves *buf and its contents as they were.  `what`: the start of the error text of a failed copy.
// `mirror`: a host copy of the contents to take them from (else device to device, from the old buffer).
template <typename T>
int grow_keep(hvs_ctx* c, T** buf, size_t want, size_t keep, const char* what, const T* mirror = nullptr)
{
    T* bigger = nullptr;
    HVS_HIP(c, hipMalloc(reinterpret_cast<void**>(&bigger), want * sizeof(T)));
    const hipMemcpyKind kind = mirror ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    hipError_t e = keep ? hipMemcpyAsync(bigger, mirror ? mirror : *buf, keep * sizeof(T), kind, c->stream) : hipSuccess;
    if (keep && e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        (void)hipFree(bigger);
        return fail(c, HVS_EHIP, std::string(what) + hipGetErrorString(e));
    }
    if (*buf) (void)hipFree(*buf);
    *buf = bigger;
    return HVS_OK;
}

std::vector<uint64_t> all_live_words(uint32_t n)
{
    std::vector<uint64_t> w(mask_words(n));
    for (size_t i = 0; i < w.size(); ++i) w[i] = masked_word(nullptr, n, i);
    return w;
}

// the device table of the k padding ids (the last k live rows, descending)
int refresh_pad_ids(hvs_ctx* c)
{
    if (!c->rs.d_pad_ids || c->rs.h_live.empty()) return HVS_OK;
    uint32_t pad[HVS_KMAX];
    hvs_mask_plan(c->rs.h_live.data(), c->n, c->k, 1.0f, nullptr, nullptr, pad);
    HVS_HIP(c, hipMemcpyAsync(c->rs.d_pad_ids, pad, (size_t)c->k * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HVS_HIP(c, hipStreamSynchronize(c->stream));  // (`pad` is on this stack)
    return HVS_OK;
}

// The index-validity mask of a context with stale rows (HvsRowSet::d_ilive), from the host's mask and stale list; room for it
// was secured by leaf_update_prepare.  No stale rows: nothing to do, index_mask(c) is d_live.
int refresh_index_mask(hvs_ctx* c)
{
    const HvsRowSet& s = c->rs;
    if (s.h_stale.empty()) return HVS_OK;
    const size_t W = 2u * mask_words(c->n_indexed);
    if (!s.d_ilive || 2u * W > s.ilive_cap) return fail(c, HVS_ESTATE, "internal: no room for the index-validity mask");
    std::vector<uint32_t> w(2u * W, 0u);
    for (size_t i = 0; i < W; ++i) w[i] = w[W + i] = (i >> 1) < s.h_live.size() ? mask_half(s.h_live[i >> 1], i) : 0u;
    const size_t last = W / 2u - 1u;  // (the bits of the tail's rows in the last word are not the index's business)
    for (size_t i = 2u * last; i < W && last < s.h_live.size(); ++i) w[i] = w[W + i] = mask_half(masked_word(s.h_live.data(), c->n_indexed, last), i);
    for (uint32_t id : s.h_stale) w[id >> 5] &= ~(1u << (id & 31u));
    HVS_HIP(c, hipMemcpyAsync(s.d_ilive, w.data(), w.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HVS_HIP(c, hipStreamSynchronize(c->stream));  // (`w` goes with this scope)
    return HVS_OK;
}

// What follows from a change of the row set, each case in this order (the table of DESIGN 3.9a); the caller has written the new
// h_live / n_dead / h_stale / n.  MaskLostRows is also a mask set anew with no row changed.
enum class RowChange { MaskLostRows, MaskRevivedRows, StaleGrew, RowsAppended, Renumbered };
int row_set_changed(hvs_ctx* c, RowChange ch)
{
    HvsRowSet& s = c->rs;
    int rc;
    switch (ch) {
    case RowChange::MaskLostRows:
    case RowChange::MaskRevivedRows:  // (tiles: rebuilt, which patches at its end, or patched; nothing without tiles)
        s.cut_valid = s.lp_valid = false;
        if ((rc = refresh_index_mask(c))) return rc;
        rc = ch == RowChange::MaskRevivedRows && c->fmt.built != HVS_FMT_NONE ? build_tiles(c, c->fmt.built) : patch_tiles(c);
        return rc ? rc : refresh_pad_ids(c);
    case RowChange::StaleGrew:  // (a stale row is live: the mask, the cut and the padding ids stand)
        s.lp_valid = false;
        return (rc = refresh_index_mask(c)) ? rc : patch_tiles(c);
    case RowChange::RowsAppended:  // (counts, index mask and tiles cover indexed rows only)
        s.cut_valid = false;
        return refresh_pad_ids(c);
    case RowChange::Renumbered:  // (reset_row_set: no mask and no stale row, and the caller re-indexes)
        s.cut_valid = s.lp_valid = false;
    }
    return HVS_OK;
}

// The row-set state of a fresh load: every row live and no mask set (the next mask call allocates d_live for the rows there
// are then), no stale row (its device buffers stay), no index attempted, nothing cached.  n, n_cap and D are the caller's:
// a load (begin_data) or a compaction (leaf_compact_commit); what the two do differently is written at each call.
int reset_row_set(hvs_ctx* c)
{
    HvsRowSet& s = c->rs;
    s.h_live.clear();
    s.h_stale.clear();
    s.n_dead = s.index_tried_n = s.live_cap = 0;
    const int rc = dev_alloc(c, &s.d_live, (size_t)0);
    return rc ? rc : row_set_changed(c, RowChange::Renumbered);
}

int begin_data(hvs_ctx* c, uint32_t n)
{
    if (n < c->k) return fail(c, HVS_EINVAL, "data set needs at least k (default 100) rows (the reference pads results with rows n-1, n-2, ...)");
    int rc = begin_mutation(c);
    if (rc) return rc;
    c->n = c->rs.n_cap = 0;
    if ((rc = reset_row_set(c))) return rc;
    // ... and drops the shared row sets with the indices that name them: they described the rows that go
    c->rs.drop_sets();
    c->qs.rset_set = false;
    // a load, unlike a compaction, starts the figures of the data set over (the tail limit is a setting and stays) ...
    c->rs.reindexes = 0;
    c->rs.reindex_ms = 0.0;
    c->rs.cstat = hvs_compact_info{};
    // ... and frees the live-row counts along the orderings itself (a compaction leaves that to leaf_reindex)
    if ((rc = dev_alloc(c, &c->ord[0].lp, (size_t)0))) return rc;
    if ((rc = dev_alloc(c, &c->ord[1].lp, (size_t)0))) return rc;
    if ((rc = dev_alloc(c, &c->d_data, (size_t)n * HVS_DCOLS))) return rc;
    c->rs.n_cap = n;
    return HVS_OK;
}

// upload/generation is timed by ev_q0..ev_q1; the index build (orderings + tiles) follows
int index_data(hvs_ctx* c);
int finish_data(hvs_ctx* c)
{
    float ms = 0.f;
    HVS_HIP(c, hipEventElapsedTime(&ms, c->call.ev_q0, c->call.ev_q1));
    c->load_ms = ms;
    return index_data(c);
}

// the index over all rows of D as they are now: at the end of a load, and again when appended rows are folded in (reindex)
int index_data(hvs_ctx* c)
{
    float ms = 0.f;
    free_index(c);
    // the index (two orderings + tiles) serves both engines: the exact engine scans position ranges
    if (c->n < kIndexMinRows && !is_filter_engine(c->engine)) return HVS_OK;
    c->rs.index_tried_n = c->n;
    HVS_HIP(c, hipEventRecord(c->call.ev_q0, c->stream));
    int rc = build_index(c);
    if (rc == HVS_ENOMEM) {
        // not enough HBM for the index next to D: the data set stays usable through the exact engine
        (void)hipGetLastError();
        free_index(c);
        c->err = "index not built (out of device memory): exact engine only";
        rc = HVS_OK;
    }
    if (rc) return rc;
    HVS_HIP(c, hipEventRecord(c->call.ev_q1, c->stream));
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    HVS_HIP(c, hipEventElapsedTime(&ms, c->call.ev_q0, c->call.ev_q1));
    c->index_ms = ms;
    c->load_ms += ms;
    trace_mark(c, "index");
    if (c->reserve_nq) {  // the caller announced its call size (hvs_reserve)
        // not fatal: D and the index are loaded; the first query allocates what it needs (or reports the failure itself)
        if (leaf_reserve(c, c->reserve_nq) == HVS_ENOMEM) {
            (void)hipGetLastError();
            c->err = "batch workspace not reserved (out of device memory): allocated by the first query";
        }
    }
    return HVS_OK;
}

bool host_pointer_is_pinned(const void* p)
{
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();  // ordinary (pageable) host memory is "invalid value" to this query
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

// H2D of rows into c->d_data (or any device buffer), from pageable or pinned host memory.  Pageable sources go
// through the pinned ring in 27 MB pieces so that the host copy of piece i+1 overlaps the DMA of piece i
// (reference io.h:111-136 is replaced by the caller's bulk read; this replaces the staging an H2D of pageable memory
// would do inside the runtime, at roughly twice its rate).
int upload_rows(hvs_ctx* c, float* dst, const float* src, size_t nfloats)
{
    if (nfloats == 0) return HVS_OK;
    if (host_pointer_is_pinned(src)) {
        HVS_HIP(c, hipMemcpyAsync(dst, src, nfloats * sizeof(float), hipMemcpyHostToDevice, c->stream));
        return HVS_OK;
    }
    // (in units of query rows: 104 floats; data rows move through the same slots)
    int rc = c->pipe.size_for(c->k, false, (nfloats + HVS_QCOLS - 1u) / HVS_QCOLS, 0u);
    const size_t slot = (size_t)HvsCopyPipe::kStageQ * HVS_QCOLS;  // floats per slot
    size_t off = 0;
    for (uint32_t piece = 0; !rc && off < nfloats; ++piece, off += slot)
        rc = c->pipe.stage_in(dst + off, src + off, std::min(slot, nfloats - off) * sizeof(float), piece);
    return rc ? rc : c->pipe.wait_in();
}

// upload only (the multi-GPU root lets the other GPUs copy D from this one while it builds its index)
int leaf_upload_data(hvs_ctx* c, const float* rows, uint32_t n)
{
    int rc = begin_data(c, n);
    if (rc) return rc;
    trace_mark(c, "alloc");
    HVS_HIP(c, hipEventRecord(c->call.ev_q0, c->stream));
    if ((rc = upload_rows(c, c->d_data, rows, (size_t)n * HVS_DCOLS))) return rc;
    HVS_HIP(c, hipEventRecord(c->call.ev_q1, c->stream));
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    c->n = n;
    return HVS_OK;
}

int leaf_load_data(hvs_ctx* c, const float* rows, uint32_t n)
{
    HostTrace tr;
    c->trace = &tr;
    int rc = leaf_upload_data(c, rows, n);
    trace_mark(c, "upload");
    if (!rc) rc = finish_data(c);
    trace_mark(c, "done");
    tr.flush("hvs_load_data", n);
    c->trace = nullptr;
    return rc;
}

// D replicated from another GPU's copy (xGMI peer copy; same-device contexts: a device-to-device copy)
int leaf_load_data_from_peer(hvs_ctx* c, const hvs_ctx* src)
{
    const uint32_t n = src->n;
    int rc = begin_data(c, n);
    if (rc) return rc;
    HVS_HIP(c, hipEventRecord(c->call.ev_q0, c->stream));
    HVS_HIP(c, hipMemcpyPeerAsync(c->d_data, c->device, src->d_data, src->device, (size_t)n * HVS_DCOLS * sizeof(float), c->stream));
    HVS_HIP(c, hipEventRecord(c->call.ev_q1, c->stream));
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    c->n = n;
    return finish_data(c);
}

// ---- inputs from device memory (include/hvs.h "device-resident inputs") ----
// A caller's buffer: plain device memory of a visible GPU (its index goes to *dev), anywhere inside an allocation.  Host memory
// -- pageable, pinned or managed -- is refused before anything changes, and the runtime's error for a pointer it does not know
// is taken off HIP's last-error slot.
int device_of_buffer(hvs_ctx* c, const void* p, const char* fn, int* dev)
{
    hipPointerAttribute_t a{};
    const hipError_t e = hipPointerGetAttributes(&a, p);
    if (e != hipSuccess) (void)hipGetLastError();
    if (e != hipSuccess || a.type != hipMemoryTypeDevice || a.isManaged)
        return fail(c, HVS_EINVAL, std::string(fn) + ": the buffer is not plain device memory (host, pinned and managed memory go through the host entry points)");
    *dev = a.device;
    return HVS_OK;
}

// ... and the work the caller has enqueued on `stream` (a stream of that GPU; NULL: its null stream) is complete: the buffer
// holds what the copies are about to read.  A host wait: the calls block until their copies are done anyway.
int wait_for_producer(hvs_ctx* c, int dev, void* stream)
{
    HVS_HIP(c, hipSetDevice(dev));
    HVS_HIP(c, hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return HVS_OK;
}

// `bytes` from a device buffer of GPU `src_dev` to this context's GPU, on its stream (same GPU: a device-to-device copy)
int copy_from_device(hvs_ctx* c, void* dst, const void* src, int src_dev, size_t bytes)
{
    if (bytes) HVS_HIP(c, hipMemcpyPeerAsync(dst, c->device, src, src_dev, bytes, c->stream));
    return HVS_OK;
}

// a caller's array to this context's GPU, on its stream: from host memory (src_dev < 0) or from device memory of GPU src_dev
int copy_in(hvs_ctx* c, void* dst, const void* src, int src_dev, size_t bytes)
{
    if (src_dev >= 0) return copy_from_device(c, dst, src, src_dev, bytes);
    if (bytes) HVS_HIP(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    return HVS_OK;
}

// hvs_load_data_device: leaf_load_data_from_peer with the caller's buffer in the place of a peer's D
int leaf_load_data_device(hvs_ctx* c, const float* d_rows, int src_dev, uint32_t n)
{
    int rc = begin_data(c, n);
    if (rc) return rc;
    HVS_HIP(c, hipEventRecord(c->call.ev_q0, c->stream));
    if ((rc = copy_from_device(c, c->d_data, d_rows, src_dev, (size_t)n * HVS_DCOLS * sizeof(float)))) return rc;
    HVS_HIP(c, hipEventRecord(c->call.ev_q1, c->stream));
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    c->n = n;
    return finish_data(c);
}

// (`first_row`: the place of the context's row 0 in the gen-v1 stream -- a part of a row-partitioned context)
int leaf_gen_data(hvs_ctx* c, uint32_t n, uint64_t seed, int profile, uint32_t ncat, uint64_t first_row = 0)
{
    int rc = begin_data(c, n);
    if (rc) return rc;
    HVS_HIP(c, hipEventRecord(c->call.ev_q0, c->stream));
    hipLaunchKernelGGL(hvs_k_gen_data, dim3(256 * 8), dim3(256), 0, c->stream, c->d_data, (uint64_t)n * HVS_DCOLS,
                       seed, profile, ncat, first_row);
    HVS_HIP(c, hipGetLastError());
    HVS_HIP(c, hipEventRecord(c->call.ev_q1, c->stream));
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    c->n = n;
    return finish_data(c);
}

int leaf_begin_queries(hvs_ctx* c, uint32_t nq)
{
    HVS_HIP(c, hipSetDevice(c->device));
    int rc = resolve_overflow(c);
    if (rc) return rc;
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    c->nq = 0;
    resident_set_replaced(c);
    return ensure_queries(c, nq);
}

// ---- attaching per-query values to the resident queries (HvsQuerySet) ----
enum class PerQuery { Caps, Cursors };
// Where the values come from.  `f`: the caps, or the cursors' distances; `u`: the cursors' ids.
struct PerQuerySource {
    enum Kind {
        Remove,    // nothing: the values are taken off
        Host,      // host memory
        Device,    // device buffers of GPU `dev` (checked and waited for by the caller)
        LastSlot,  // cursors only: slot k-1 of the result rows f (distances) / u (ids), k slots each
        InPlace    // cursors only: the raw pairs are in the arrays already (a row-partitioned context's exchange put them there)
    } kind = Remove;
    const float* f = nullptr;
    const uint32_t* u = nullptr;
    int dev = -1;
};
// a caller's arrays: host memory (src_dev < 0) or device memory of GPU src_dev; f == nullptr: remove
PerQuerySource caller_values(const float* f, const uint32_t* u, int src_dev)
{
    return PerQuerySource{!f ? PerQuerySource::Remove : src_dev < 0 ? PerQuerySource::Host : PerQuerySource::Device, f, u, src_dev};
}

// room for `nq` cursors in the engines' arrays (allocated by the first call that sets any: contexts that never page pay nothing)
int ensure_after(hvs_ctx* c, uint32_t nq)
{
    if (nq <= c->qs.eng.after_cap) return HVS_OK;
    c->qs.after_set = false;  // (the buffers are about to change hands)
    return per_query_room(c, c->qs.eng, kCursors, nq);
}

// Exclusion lists without cursors run the cursor forms of the kernels: an after_lo of zeros, one per resident
// query, admits every key.  Called whenever lists are (or stay) set while cursors are not.
int zero_after_lo(hvs_ctx* c)
{
    if (int rc = ensure_after(c, std::max(c->nq, 1u))) return rc;
    HVS_HIP(c, hipMemsetAsync(c->qs.eng.d_after_lo, 0, (size_t)c->qs.eng.after_cap * sizeof(uint64_t), c->stream));
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    return HVS_OK;
}

// ---- the staged attach: two steps per GPU, so that a refusal on any GPU leaves every GPU as it was ----
// Step 1, the same for every kind: `words` of the caller's (host memory, src_dev < 0, or device memory of GPU src_dev) into the
// staging area `st` and through the kind's check kernel -- `check(st)` enqueues it --, and the status block back into st.flags /
// first / end.  Nothing that is in force is touched.  An earlier call's re-runs are resolved first, under what they were asked
// under; `expanded`: the words are a client's of the expanded set, which begins as every change of that set does (in_begin).
int in_begin(hvs_ctx* c);
template <typename Check>
int leaf_stage(hvs_ctx* c, HvsStage& st, bool expanded, const uint32_t* src, int src_dev, uint32_t words, Check check)
{
    int rc;
    if (expanded)
        rc = in_begin(c);
    else {
        HVS_HIP(c, hipSetDevice(c->device));
        rc = resolve_overflow(c);
    }
    if (rc || (rc = ensure_room(c, &st.d_words, st.cap, std::max(words, 1u)))) return rc;
    if (!st.d_status && (rc = dev_alloc(c, &st.d_status, (size_t)4))) return rc;
    if ((rc = copy_in(c, st.d_words, src, src_dev, (size_t)words * sizeof(uint32_t)))) return rc;
    HVS_HIP(c, hipMemsetAsync(st.d_status, 0, 4 * sizeof(uint32_t), c->stream));
    if ((rc = check(st))) return rc;
    uint32_t h[4] = {0, 0, 0, 0};
    HVS_HIP(c, hipMemcpyAsync(h, st.d_status, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    st.flags = h[0], st.first = h[1], st.end = h[2];
    return HVS_OK;
}
// the check of `count` + 1 staged CSR offsets: no list longer than `limit`; `first`: they are the head of the caller's array
int check_offsets(hvs_ctx* c, const HvsStage& st, uint32_t count, bool first, uint32_t limit)
{
    hipLaunchKernelGGL(hvs_k_check_offsets, dim3(hvs_ceil_div(std::max(count, 1u), 256u)), dim3(256), 0, c->stream, st.d_words, count, first ? 1 : 0,
                       limit, st.d_status);
    HVS_HIP(c, hipGetLastError());
    return HVS_OK;
}

// ---- per-query id lists: exclusion lists and candidate lists ----
// What tells the two kinds apart: the limit of the offsets' check, the normalisation kernel and its queries per workgroup, where
// the lists and their index live, and what composes -- exclusion lists are the user's under the expanded set (every sub-query
// takes its parent's pair) and are read by cursor forms (zero_after_lo); candidate lists are neither.
struct ListKind {
    uint32_t limit;
    void (*norm)(const uint32_t*, uint32_t, uint32_t*, uint32_t, uint32_t, uint32_t*, uint32_t*);
    uint32_t queries_per_block;
    HvsIdLists HvsQuerySet::*lists;
    int flag;                // HvsQuerySet::Attachment
    bool cursor_forms;       // expanded under in.active, zero_after_lo follows
    const char *offsets, *too_long;  // of the refusals: the parameter's name, the limit's text
};
const ListKind kExcludeLists{HVS_EXCLUDE_MAX_, hvs_k_norm_exclude, 4u, &HvsQuerySet::excl, HvsQuerySet::kExclOn, true, "excl_offsets",
                             ": a list has more than HVS_EXCLUDE_MAX entries"};
const ListKind kCandidateLists{HVS_CANDIDATES_MAX_, hvs_k_norm_candidates, 1u, &HvsQuerySet::cand, HvsQuerySet::kCandOn, false, "cand_offsets",
                               ": a list has more than HVS_CANDIDATES_MAX entries"};

// Step 1 for lists: `count` + 1 offsets; `first`: they are the head of the caller's array
int leaf_lists_stage(hvs_ctx* c, const ListKind& K, const uint32_t* off, int src_dev, uint32_t count, bool first)
{
    return leaf_stage(c, c->qs.off_stage, false, off, src_dev, count + 1u, [&](const HvsStage& st) { return check_offsets(c, st, count, first, K.limit); });
}
// Step 2 (every GPU's offsets were accepted): the ids behind the staged offsets -- `ids` is the caller's array -- are copied
// and normalised in place for rows [row0, row0 + n_rows) by the kind's kernel; exclusion lists under category sets are the
// user's, and every sub-query takes its parent's pair.
int leaf_lists_commit(hvs_ctx* c, const ListKind& K, const uint32_t* ids, int src_dev, uint32_t count, uint32_t row0, uint32_t n_rows)
{
    HvsQuerySet& s = c->qs;
    HvsIdLists& L = s.*K.lists;
    const bool sets = K.cursor_forms && s.in.active;
    HvsListIndex& at = !K.cursor_forms ? s.cand_at : sets ? s.in.user.ex : s.eng.ex;
    int rc;
    HVS_HIP(c, hipSetDevice(c->device));
    L.set = false;  // (the buffers are about to change)
    if ((rc = ensure_room(c, &at.d_begin, at.cap, std::max(count, 1u), &at.d_count)) ||
        (sets && (rc = ensure_room(c, &s.eng.ex.d_begin, s.eng.ex.cap, std::max(c->nq, 1u), &s.eng.ex.d_count))))
        return rc;
    const uint32_t total = s.off_stage.total();
    if ((rc = ensure_room(c, &L.d_ids, L.ids_cap, std::max(total, 1u))) ||
        (rc = copy_in(c, L.d_ids, ids + s.off_stage.first, src_dev, (size_t)total * sizeof(uint32_t))))
        return rc;
    if (count) {
        hipLaunchKernelGGL(K.norm, dim3(hvs_ceil_div(count, K.queries_per_block)), dim3(256), 0, c->stream, s.off_stage.d_words, count, L.d_ids, row0, n_rows,
                           at.d_begin, at.d_count);
        HVS_HIP(c, hipGetLastError());
        if (sets && c->nq) {
            hipLaunchKernelGGL(hvs_k_expand_exclude, dim3(hvs_ceil_div(c->nq, 256u)), dim3(256), 0, c->stream, s.in.d_parent, c->nq, at.d_begin, at.d_count,
                               s.eng.ex.d_begin, s.eng.ex.d_count);
            HVS_HIP(c, hipGetLastError());
        }
    }
    if (K.cursor_forms && !s.after_set && (rc = zero_after_lo(c))) return rc;
    HVS_HIP(c, hipStreamSynchronize(c->stream));  // (the caller's buffers are the caller's again)
    L.nq = count;
    L.total = total;
    L.set = true;
    return HVS_OK;
}
// lists or set indices off one GPU's queries: an earlier call's re-runs are resolved under them, then the flag goes
int leaf_detach_flag(hvs_ctx* c, int attachment)
{
    HVS_HIP(c, hipSetDevice(c->device));
    if (int rc = resolve_overflow(c)) return rc;
    c->qs.attached(attachment) = false;
    return HVS_OK;
}

// ---- shared row sets ----
// rows this GPU's bitmaps cover (a part of a row-partitioned context: the whole D's), and the u32 words of one set over `rows` rows
uint32_t set_rows(const hvs_ctx* c) { return c->rs.sets_part_rows ? c->rs.sets_part_rows : c->n; }
uint32_t set_words_for(uint32_t rows) { return (uint32_t)(mask_words(rows) * 2u); }
dim3 set_grid(uint64_t words) { return dim3((uint32_t)std::min<uint64_t>(std::max<uint64_t>((words + 255u) / 256u, 1u), 65535u)); }

// n_sets bitmaps of `words` words each into a fresh rs.d_sets_next, taken from `src` (src_words words each: device memory of this
// GPU, or nullptr = all sets empty) with the bits at or past `rows` cleared.  Nothing in force changes.
int sets_build_next(hvs_ctx* c, const uint32_t* src, uint32_t src_words, uint32_t n_sets, uint32_t words, uint32_t rows)
{
    HvsRowSet& s = c->rs;
    HvsRowSet::drop(s.d_sets_next);
    const size_t total = (size_t)n_sets * words;
    HVS_HIP(c, hipMalloc(reinterpret_cast<void**>(&s.d_sets_next), std::max<size_t>(total, 1u) * sizeof(uint32_t)));
    if (!src) {
        HVS_HIP(c, hipMemsetAsync(s.d_sets_next, 0, total * sizeof(uint32_t), c->stream));
    } else {
        hipLaunchKernelGGL(hvs_k_row_sets_restride, set_grid(total), dim3(256), 0, c->stream, src, src_words, s.d_sets_next, words, n_sets, rows);
        HVS_HIP(c, hipGetLastError());
    }
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    return HVS_OK;
}
// ... and d_sets_next takes d_sets' place
void sets_swap_next(hvs_ctx* c, uint32_t n_sets, uint32_t words)
{
    HvsRowSet& s = c->rs;
    HvsRowSet::drop(s.d_sets);
    s.d_sets = s.d_sets_next;
    s.d_sets_next = nullptr;
    s.n_sets = n_sets;
    s.sets_words = words;
}
// the sets as they are, re-strided to `words` words each (capacity growth, trim): prepare, then sets_swap_next
int sets_restride_next(hvs_ctx* c, uint32_t words)
{
    return sets_build_next(c, c->rs.d_sets, c->rs.sets_words, c->rs.n_sets, words, set_rows(c));
}

// hvs_set_row_sets on one GPU, first half: the caller's bitmaps (host memory, src_dev < 0, or device memory of GPU src_dev;
// nullptr: empty sets) over `rows` rows into d_sets_next.  `part_rows` != 0: this GPU is a part, the bitmaps cover the whole D.
int leaf_row_sets_prepare(hvs_ctx* c, const uint64_t* bits, int src_dev, uint32_t n_sets, uint32_t part_rows)
{
    int rc = begin_mutation(c);
    if (rc || n_sets == 0u) return rc;
    const uint32_t rows = part_rows ? part_rows : c->n;
    const uint32_t src_words = set_words_for(rows), words = set_words_for(part_rows ? part_rows : std::max(c->n, c->rs.n_cap));
    uint32_t* staged = nullptr;
    if (bits) {
        const size_t bytes = (size_t)n_sets * src_words * sizeof(uint32_t);
        HVS_HIP(c, hipMalloc(reinterpret_cast<void**>(&staged), bytes));
        rc = copy_in(c, staged, bits, src_dev, bytes);
    }
    if (!rc) rc = sets_build_next(c, staged, src_words, n_sets, words, rows);
    if (staged) (void)hipFree(staged);
    return rc;
}
// second half: the new sets are in force; the queries' indices named the old ones and go, and so do the results
int leaf_row_sets_commit(hvs_ctx* c, uint32_t n_sets, uint32_t part_rows, uint32_t row0)
{
    HVS_HIP(c, hipSetDevice(c->device));
    if (n_sets == 0u)
        c->rs.drop_sets();
    else {
        sets_swap_next(c, n_sets, set_words_for(part_rows ? part_rows : std::max(c->n, c->rs.n_cap)));
        c->rs.sets_part_rows = part_rows;
        c->rs.sets_row0 = row0;
    }
    c->qs.rset_set = false;
    c->qs.drop_results();
    return HVS_OK;
}

// hvs_assign_row_sets on one GPU: bits of set `set` (< n_sets: checked by the caller) from `count` host ids
int leaf_assign_row_sets(hvs_ctx* c, uint32_t set, const uint32_t* ids, uint32_t count, int member)
{
    HvsRowSet& s = c->rs;
    int rc = begin_mutation(c);  // (an earlier call's re-runs: under the sets they were asked under)
    if (rc) return rc;
    if ((rc = ensure_room(c, &s.d_sets_ids, s.sets_ids_cap, count))) return rc;
    HVS_HIP(c, hipMemcpyAsync(s.d_sets_ids, ids, (size_t)count * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(hvs_k_row_sets_assign, dim3(hvs_ceil_div(count, 256u)), dim3(256), 0, c->stream, s.d_sets_ids, count, set_rows(c),
                       s.d_sets + (size_t)set * s.sets_words, member);
    HVS_HIP(c, hipGetLastError());
    HVS_HIP(c, hipStreamSynchronize(c->stream));  // (the ids are the caller's)
    return HVS_OK;
}

int leaf_get_row_sets(hvs_ctx* c, uint64_t* bits)
{
    const HvsRowSet& s = c->rs;
    int rc = leaf_sync(c);
    if (rc) return rc;
    const size_t width = (size_t)set_words_for(set_rows(c)) * sizeof(uint32_t);
    if (width && s.n_sets)
        HVS_HIP(c, hipMemcpy2D(bits, width, s.d_sets, (size_t)s.sets_words * sizeof(uint32_t), width, s.n_sets, hipMemcpyDeviceToHost));
    return HVS_OK;
}

// The per-query set indices take the two steps of the id lists.  Step 1: `count` indices into idx_stage and through
// hvs_k_check_query_row_sets (flags: 1 = an index names no set).
int leaf_query_sets_stage(hvs_ctx* c, const uint32_t* idx, int src_dev, uint32_t count)
{
    return leaf_stage(c, c->qs.idx_stage, false, idx, src_dev, count, [&](const HvsStage& st) {
        if (!count) return HVS_OK;
        hipLaunchKernelGGL(hvs_k_check_query_row_sets, dim3(hvs_ceil_div(count, 256u)), dim3(256), 0, c->stream, st.d_words, count, c->rs.n_sets, st.d_status);
        HVS_HIP(c, hipGetLastError());
        return HVS_OK;
    });
}
// Step 2 (every GPU's indices were accepted): the staged indices are the queries'; under the expanded set they are the user's, and
// every sub-query takes its parent's.
int leaf_query_sets_commit(hvs_ctx* c, uint32_t count)
{
    HvsQuerySet& s = c->qs;
    const bool sets = s.in.active;
    HvsPerQuery& dst = sets ? s.in.user : s.eng;
    int rc;
    HVS_HIP(c, hipSetDevice(c->device));
    s.rset_set = false;  // (the buffers are about to change)
    if ((rc = ensure_room(c, &dst.d_set_of, dst.set_of_cap, std::max(count, 1u))) ||
        (sets && (rc = ensure_room(c, &s.eng.d_set_of, s.eng.set_of_cap, std::max(c->nq, 1u)))) ||
        (rc = ensure_room(c, &s.d_rs_zero, s.rs_zero_cap, std::max(c->nq, 1u))))
        return rc;
    HVS_HIP(c, hipMemsetAsync(s.d_rs_zero, 0, (size_t)s.rs_zero_cap * sizeof(uint32_t), c->stream));
    if (count) {
        HVS_HIP(c, hipMemcpyAsync(dst.d_set_of, s.idx_stage.d_words, (size_t)count * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
        if (sets && c->nq) {
            hipLaunchKernelGGL(hvs_k_expand_query_row_sets, dim3(hvs_ceil_div(c->nq, 256u)), dim3(256), 0, c->stream, s.in.d_parent, c->nq, dst.d_set_of,
                               s.eng.d_set_of);
            HVS_HIP(c, hipGetLastError());
        }
    }
    if (!s.after_set && !s.excl.set && (rc = zero_after_lo(c))) return rc;  // (under lists without cursors it holds zeros already)
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    s.rset_set = true;
    return HVS_OK;
}

// The one way caps or cursors reach the resident queries of one GPU: `count` values from `src` (count = the user's resident
// queries: checked by the caller) are attached, or the values are removed.  Under category sets they are the user's, one per user
// query: copied and normalised on the user's side (HvsInSet::user), then every sub-query takes its parent's.  `row0` (cursors):
// the first global row of this GPU's part.  An earlier call's pending re-runs are resolved first, under the values they were
// asked under; results of earlier calls stay.  The call returns when the caller's buffers are the caller's again.
int leaf_attach(hvs_ctx* c, PerQuery what, const PerQuerySource& src, uint32_t count, uint32_t row0)
{
    HvsQuerySet& s = c->qs;
    const bool caps = what == PerQuery::Caps, sets = s.in.active;
    int rc;
    if (src.kind != PerQuerySource::InPlace) {
        HVS_HIP(c, hipSetDevice(c->device));
        if ((rc = resolve_overflow(c))) return rc;  // (for LastSlot: the last slots of re-run queries too)
        if (src.kind == PerQuerySource::Remove) {
            (caps ? s.caps_set : s.after_set) = false;
            if (!caps && (s.excl.set || s.rset_set)) return zero_after_lo(c);  // (the list forms are cursor forms: they go on reading after_lo)
            return HVS_OK;
        }
        if (!caps && (rc = ensure_after(c, std::max(std::max(count, sets ? c->nq : 0u), 1u)))) return rc;  // (under sets: room for every sub-query)
    }
    if (count) {
        const HvsPerQuery& dst = sets ? s.in.user : s.eng;
        const dim3 grid(hvs_ceil_div(count, 256u)), sub_grid(hvs_ceil_div(c->nq, 256u));
        auto copy = [&](void* to, const void* from, size_t bytes) { return copy_in(c, to, from, src.kind == PerQuerySource::Device ? src.dev : -1, bytes); };
        if (caps) {
            if ((rc = copy(dst.d_max_d2, src.f, (size_t)count * sizeof(float)))) return rc;
            hipLaunchKernelGGL(hvs_k_norm_caps, grid, dim3(256), 0, c->stream, dst.d_max_d2, count);
            HVS_HIP(c, hipGetLastError());
            if (sets)
                hipLaunchKernelGGL(hvs_k_expand_per_query, sub_grid, dim3(256), 0, c->stream, s.in.d_parent, c->nq, dst.d_max_d2, s.eng.d_max_d2, nullptr,
                                   nullptr, nullptr, nullptr, nullptr, nullptr);
        } else {
            if (src.kind == PerQuerySource::LastSlot) {
                hipLaunchKernelGGL(hvs_k_after_from_results, grid, dim3(256), 0, c->stream, src.u, src.f, count, c->k, dst.d_after_dist, dst.d_after_id);
                HVS_HIP(c, hipGetLastError());
            } else if (src.kind != PerQuerySource::InPlace) {
                if ((rc = copy(dst.d_after_dist, src.f, (size_t)count * sizeof(float))) || (rc = copy(dst.d_after_id, src.u, (size_t)count * sizeof(uint32_t))))
                    return rc;
            }
            hipLaunchKernelGGL(hvs_k_norm_after, grid, dim3(256), 0, c->stream, dst.d_after_dist, dst.d_after_id, count, row0, dst.d_after_lo);
            if (sets)
                hipLaunchKernelGGL(hvs_k_expand_per_query, sub_grid, dim3(256), 0, c->stream, s.in.d_parent, c->nq, nullptr, nullptr, dst.d_after_lo,
                                   dst.d_after_dist, dst.d_after_id, s.eng.d_after_lo, s.eng.d_after_dist, s.eng.d_after_id);
        }
        if (!caps || sets) HVS_HIP(c, hipGetLastError());
    }
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    (caps ? s.caps_set : s.after_set) = true;
    return HVS_OK;
}

// hvs_set_after_from_results on one GPU that holds its own results (a single context, a leaf of a replicated one): checked by
// the caller -- results of all resident queries exist with the current k, padding is off.  Under category sets: slot k-1 of the
// MERGED rows, one cursor per user query.
int leaf_after_from_results(hvs_ctx* c)
{
    return leaf_attach(c, PerQuery::Cursors, PerQuerySource{PerQuerySource::LastSlot, user_dists(c), user_ids(c), -1}, user_nq(c), 0u);
}

int leaf_upload_queries(hvs_ctx* c, const float* q_rows, uint32_t nq)
{
    int rc = leaf_begin_queries(c, nq);
    if (rc) return rc;
    if ((rc = upload_rows(c, c->d_q, q_rows, (size_t)nq * HVS_QCOLS))) return rc;
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    c->nq = nq;
    return HVS_OK;
}

// hvs_set_queries_device: the same from a device buffer of GPU `src_dev` (checked and waited for by the caller)
int leaf_set_queries_device(hvs_ctx* c, const float* d_q_rows, int src_dev, uint32_t nq)
{
    int rc = leaf_begin_queries(c, nq);
    if (rc) return rc;
    if ((rc = copy_from_device(c, c->d_q, d_q_rows, src_dev, (size_t)nq * HVS_QCOLS * sizeof(float)))) return rc;
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    c->nq = nq;
    return HVS_OK;
}

// hvs_set_queries_from_rows: query j from row ids[j] (ids == nullptr: row first_id + j) of D as it is now; ids, type and dt
// checked by the caller.  The id list travels through the staging buffer of hvs_delete_rows' id lists.
int leaf_set_queries_from_rows(hvs_ctx* c, const uint32_t* ids, uint32_t first_id, uint32_t nq, int type, float dt)
{
    HvsRowSet& s = c->rs;
    int rc = leaf_begin_queries(c, nq);
    if (rc) return rc;
    if (nq) {
        if (ids) {
            if ((rc = ensure_room(c, &s.d_mask_ids, s.mask_ids_cap, nq))) return rc;
            HVS_HIP(c, hipMemcpyAsync(s.d_mask_ids, ids, (size_t)nq * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        }
        hipLaunchKernelGGL(hvs_k_queries_from_rows, dim3(hvs_ceil_div(nq, 4u * HVS_ROWQ_WAVE_ROWS)), dim3(256), 0, c->stream,
                           reinterpret_cast<const uint2*>(c->d_data), ids ? s.d_mask_ids : nullptr, first_id, nq, type, dt,
                           reinterpret_cast<uint2*>(c->d_q));
        HVS_HIP(c, hipGetLastError());
    }
    HVS_HIP(c, hipStreamSynchronize(c->stream));  // (the id list is the caller's)
    c->nq = nq;
    return HVS_OK;
}

int leaf_gen_queries(hvs_ctx* c, uint32_t nq, uint64_t seed, int profile, uint32_t ncat, int force_type, uint64_t first_row)
{
    int rc = leaf_begin_queries(c, nq);
    if (rc) return rc;
    if (nq) {
        hipLaunchKernelGGL(hvs_k_gen_queries, dim3(256 * 4), dim3(256), 0, c->stream, c->d_q, (uint64_t)nq * HVS_QCOLS,
                           seed, profile, ncat, force_type, first_row);
        HVS_HIP(c, hipGetLastError());
    }
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    c->nq = nq;
    return HVS_OK;
}

int leaf_sync(hvs_ctx* c)
{
    HVS_HIP(c, hipSetDevice(c->device));
    int rc = resolve_overflow(c);
    if (rc) return rc;
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    return HVS_OK;
}

int leaf_download_results(hvs_ctx* c, uint32_t q0, uint32_t nq, uint32_t* out_ids, float* out_dists)
{
    if (!out_ids || (uint64_t)q0 + nq > user_nq(c)) return fail(c, HVS_EINVAL, "hvs_download_results: bad range");
    int rc = leaf_sync(c);
    if (rc) return rc;
    if (c->qs.in.active && c->qs.in.m_cap < (size_t)c->qs.in.nuq * c->k) return fail(c, HVS_ESTATE, "hvs_download_results: no results (hvs_query_resident has not run)");
    HVS_HIP(c, hipMemcpyAsync(out_ids, user_ids(c) + (size_t)q0 * c->k, (size_t)nq * c->k * sizeof(uint32_t),
                              hipMemcpyDeviceToHost, c->stream));
    if (out_dists)
        HVS_HIP(c, hipMemcpyAsync(out_dists, user_dists(c) + (size_t)q0 * c->k,
                                  (size_t)nq * c->k * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    return HVS_OK;
}

// ---- category sets (include/hvs.h "category sets"): the user's side of an expanded resident set ----

// hvs_in_plan's arithmetic; `types`: the queries' type floats, `stride` floats apart (nullptr: every query tests C), `own_v`
// likewise their own v (nullptr: none known).  A value names the category the engines would read from it (hvs_parse_query).
uint32_t in_plan_core(const float* types, const float* own_v, size_t stride, const uint32_t* off, const float* vals, uint32_t nq, uint32_t* sub_off,
                      uint32_t* parent, float* value, uint8_t* eff)
{
    if (nq && !off) return 0xFFFFFFFFu;
    if (nq && off[0] != 0u) return 0xFFFFFFFFu;
    for (uint32_t p = 0; p < nq; ++p)
        if (off[p + 1] < off[p]) return 0xFFFFFFFFu;
    if (nq && off[nq] && !vals) return 0xFFFFFFFFu;
    const float nan = __builtin_nanf("");
    // two passes: nothing is written unless the whole plan is good
    for (int pass = 0; pass < 2; ++pass) {
        uint64_t nsub = 0;
        std::vector<float> cat;
        for (uint32_t p = 0; p < nq; ++p) {
            const bool has_c = !types || hvs_in_type_has_c(types[(size_t)p * stride]);
            const bool effective = has_c && off[p + 1] > off[p];
            cat.clear();
            for (uint32_t i = off[p]; i < off[p + 1]; ++i) {
                float named;
                if (hvs_in_category(vals[i], &named)) cat.push_back(named);
            }
            std::sort(cat.begin(), cat.end());
            cat.erase(std::unique(cat.begin(), cat.end()), cat.end());
            // (the limit is the set's own: it holds whatever the query's type)
            if (cat.size() > HVS_IN_MAX_VALUES) return 0xFFFFFFFFu;
            const uint32_t m = effective ? std::max<uint32_t>((uint32_t)cat.size(), 1u) : 1u;
            if (pass) {
                if (sub_off) sub_off[p] = (uint32_t)nsub;
                if (eff) eff[p] = effective ? 1u : 0u;
                for (uint32_t j = 0; j < m; ++j) {
                    if (parent) parent[nsub + j] = p;
                    if (value) value[nsub + j] = effective ? (cat.empty() ? nan : cat[j]) : (own_v ? own_v[(size_t)p * stride] : nan);
                }
            }
            nsub += m;
        }
        if (nsub >= 0xFFFFFFFFull) return 0xFFFFFFFFu;
        if (pass) {
            if (sub_off) sub_off[nq] = (uint32_t)nsub;
            return (uint32_t)nsub;
        }
    }
    return 0u;
}

int in_ensure_events(hvs_ctx* c)
{
    for (hipEvent_t* ev : {&c->qs.in.ev_x0, &c->qs.in.ev_x1, &c->qs.in.ev_m0, &c->qs.in.ev_m1})
        if (!*ev) HVS_HIP(c, hipEventCreate(ev));
    return HVS_OK;
}

// The expanded set off one GPU, whichever client's it is: the resident set becomes the user's again (a no-op while none is attached)
int in_detach(hvs_ctx* c)
{
    HvsInSet& S = c->qs.in;
    if (!S.active) return HVS_OK;
    int rc = begin_mutation(c);
    if (rc) return rc;
    if (S.nuq) HVS_HIP(c, hipMemcpyAsync(c->d_q, S.d_uq, (size_t)S.nuq * HVS_QCOLS * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    c->nq = S.nuq;  // (nq_cap >= the sub-queries >= the user's queries)
    expanded_changed(c, false);
    return HVS_OK;
}
// ... of client K only: removing category sets leaves extra vectors alone, and the other way round
int client_detach(hvs_ctx* c, const ExpandedKind& K) { return c->qs.in.active && c->qs.in.client != &K ? HVS_OK : in_detach(c); }

// Attaching a client to one GPU's `nuq` user queries has two halves: a PLAN is made, which changes nothing a query or a later
// call reads, and in_commit puts it in force.  sub_off and eff are on the host whoever made the plan: hvs_query_resident maps
// query ranges to sub-query ranges there.  The rest of a plan is one of three payloads, and each function below takes the one
// it reads.
static_assert(HVS_INP_MAX_VALUES == HVS_IN_MAX_VALUES && HVS_IN_MAX_VALUES <= 64, "the plan kernels keep one category per lane of a wave");
struct InPlan {
    uint32_t nuq = 0, nsub = 0;
    std::vector<uint32_t> sub_off;  // nuq + 1: becomes HvsInSet::h_sub_off
    std::vector<uint8_t> eff;       // nuq: becomes HvsInSet::h_eff
    double plan_ms = 0.0;           // device time of the plan: the count and scan kernels, or the check of staged offsets
    // category sets planned on the host from a host CSR (in_plan_host): the arrays the commit uploads
    struct Host {
        std::vector<uint32_t> set_off, parent;
        std::vector<float> value;
    } host;
    // category sets planned by the plan kernels from a CSR in device memory (in_plan_device; `made`): sub_off is in
    // HvsInSet::d_p_sub_off, eff in d_p_eff, and the fill kernel reads the CSR again
    struct Device {
        bool made = false;
        const uint32_t* d_off = nullptr;  // this GPU's slice of the offsets, nuq + 1, in this GPU's memory
        const float* d_vals = nullptr;    // the values the slice points into: entry i is d_vals[i - v0]
        uint32_t v0 = 0, lo = 0;          // lo: the slice's first offset
        uint64_t sub_if_all_c = 0;        // the sub-queries there would be if every query tested C (what the limit is taken over)
    } dev;
    // extra vectors and extra clauses: the slice's offsets are staged and checked in HvsInSet::v_stage (csr_stage), and the fill
    // kernel writes sub_off and parent from them: nothing of size nsub is built on the host.  `vecs` = the first vector of the
    // slice, `attrs` = its first clause, 4 floats each: nsub - nuq of them, in host memory (src_dev < 0) or on GPU src_dev.
    // Vectors have no attrs; vecs == nullptr: predicate-only clauses.
    struct Staged {
        const float* vecs = nullptr;
        const float* attrs = nullptr;
        int src_dev = -1;
    } csr;
};

// What tells the three clients of the expanded set apart, and nothing else: category sets (3.13), extra query
// vectors (3.15) and extra clauses (3.16).  The path they share -- in_begin, a plan, in_commit, in_run, the merge's figures,
// client_detach -- reads one of the three instances below in_plan_release.
struct Refusal {
    const char *bad_first, *bad_order, *bad_long;
};
using MergeKernel = void (*)(const uint32_t*, uint32_t, uint32_t, const uint32_t*, const float*, const float*, uint32_t, const float*, int, const uint32_t*,
                             uint32_t*, float*, uint32_t, unsigned long long*);
struct ExpandedKind {
    HvsInSet::Kind kind;
    // the public names, as error texts have them: the setter and its offsets ([1]: of the _device form), the one-shot call and
    // what it says of a CSR it refuses, the stats call
    const char *set_fn[2], *offsets[2], *query_fn, *bad_query, *stats_fn;
    // How the caller's CSR becomes a plan.  `staged`: its offsets are staged in HvsInSet::v_stage, checked there against `limit`
    // extras per query and refused in the words of `why`, and its fill kernel plans (csr_stage, expanded_everywhere).  Not
    // staged: planned from its values (in_plan_host, in_plan_device), and the next five do not apply.
    bool staged;
    uint32_t limit;
    Refusal why;
    const float* InPlan::Staged::*required;  // the array extras cannot do without ...
    const char* required_null;               // ... and the refusal where it is missing
    bool vecs_optional;                      // extras need not bring vectors
    // in_commit's own two steps: what the client's kernels read reaches the device; its fill and expand launches
    int (*payload)(hvs_ctx*, const InPlan&);
    void (*expand)(hvs_ctx*, const InPlan&);
    bool (*one_key_per_row)(const InPlan&);  // -> HvsInSet::one_key_per_row
    // in_run's merge: the kernel for (summation order, list capacity); whether it pads from the user's rows or from the expanded
    // ones; how many words of HvsInSet::d_stat it counts in
    MergeKernel (*merge)(bool scalar_order, int cap);
    bool merge_user_rows;
    uint32_t stat_words;
};

// what both halves need first: an earlier call's re-runs resolved and the stream idle, the events, the merge's counters
int in_begin(hvs_ctx* c)
{
    int rc = begin_mutation(c);
    if (!rc) rc = in_ensure_events(c);
    if (!rc && !c->qs.in.d_stat) rc = dev_alloc(c, &c->qs.in.d_stat, (size_t)HvsInSet::kStatWordsMax);
    return rc;
}

// The plan of a host CSR: `off` = the caller's offsets of this GPU's `nuq` resident queries (off[0] need not be 0: a slice of a
// multi-GPU context's CSR), `vals` the whole value array; validated by the caller (format, limits, nuq = the resident queries).
// The user's rows may have come from device memory: their types are read back.
int in_plan_host(hvs_ctx* c, const uint32_t* off, const float* vals, uint32_t nuq, InPlan* P)
{
    std::vector<float> tv(2u * (size_t)nuq);  // [type, v] of every user query
    if (nuq)
        HVS_HIP(c, hipMemcpy2D(tv.data(), 2u * sizeof(float), user_queries(c), HVS_QCOLS * sizeof(float), 2u * sizeof(float), nuq, hipMemcpyDeviceToHost));
    P->nuq = nuq;
    P->host.set_off.resize((size_t)nuq + 1u);
    for (uint32_t p = 0; p <= nuq; ++p) P->host.set_off[p] = off[p] - off[0];
    const float* v0 = vals ? vals + off[0] : nullptr;
    P->sub_off.resize((size_t)nuq + 1u);
    P->eff.resize(nuq);
    P->nsub = in_plan_core(tv.data(), tv.data() + 1, 2u, P->host.set_off.data(), v0, nuq, P->sub_off.data(), nullptr, nullptr, P->eff.data());
    if (P->nsub == 0xFFFFFFFFu) return fail(c, HVS_EINVAL, "hvs_set_category_sets: malformed sets");
    P->host.parent.resize(P->nsub);
    P->host.value.resize(P->nsub);
    (void)in_plan_core(tv.data(), tv.data() + 1, 2u, P->host.set_off.data(), v0, nuq, nullptr, P->host.parent.data(), P->host.value.data(), nullptr);
    return HVS_OK;
}

// The plan of a CSR in device memory of GPU `src_dev` (checked and waited for by the caller): `d_off` = the offsets of this
// GPU's `nuq` resident queries, whose first and last, lo <= hi, the caller has read; `d_vals` the whole value array (nullptr:
// none, hi == 0).  On this GPU's own memory the kernels read both in place; from another GPU the slice of the offsets and the
// values [lo, hi) are copied here first.  What comes back to the host: the status block, sub_off and eff.  HVS_EINVAL for what
// the host plan refuses in this slice; the sum over "every query tests C" is the caller's to judge (it is context-wide).
int in_plan_device(hvs_ctx* c, const uint32_t* d_off, const float* d_vals, int src_dev, uint32_t lo, uint32_t hi, uint32_t nuq, InPlan* P)
{
    HvsInSet& S = c->qs.in;
    int rc;
    if (!S.d_p_stat || nuq > S.p_cap) {
        S.p_cap = 0;
        if ((rc = dev_alloc(c, &S.d_p_pack, (size_t)nuq)) || (rc = dev_alloc(c, &S.d_p_sub_off, (size_t)nuq + 1u)) ||
            (rc = dev_alloc(c, &S.d_p_eff, (size_t)nuq)) || (rc = dev_alloc(c, &S.d_p_stat, (size_t)3)))
            return rc;
        S.p_cap = nuq;
    }
    P->dev.made = true;
    P->nuq = nuq;
    P->dev.lo = lo;
    if (src_dev == c->device) {
        P->dev.d_off = d_off;
        P->dev.d_vals = d_vals;
        P->dev.v0 = 0u;
    } else {
        if ((rc = ensure_room(c, &S.d_p_off, S.p_off_cap, (size_t)nuq + 1u)) || (rc = ensure_room(c, &S.d_p_vals, S.pv_cap, hi - lo)) ||
            (rc = copy_from_device(c, S.d_p_off, d_off, src_dev, ((size_t)nuq + 1u) * sizeof(uint32_t))) ||
            (rc = copy_from_device(c, S.d_p_vals, d_vals ? d_vals + lo : nullptr, src_dev, d_vals ? (size_t)(hi - lo) * sizeof(float) : 0u)))
            return rc;
        P->dev.d_off = S.d_p_off;
        P->dev.d_vals = d_vals && hi > lo ? S.d_p_vals : nullptr;
        P->dev.v0 = lo;
    }
    HVS_HIP(c, hipMemsetAsync(S.d_p_stat, 0, 3u * sizeof(unsigned long long), c->stream));
    HVS_HIP(c, hipEventRecord(S.ev_x0, c->stream));
    if (nuq)
        hipLaunchKernelGGL(hvs_k_in_count, dim3((nuq + 3u) / 4u), dim3(256), 0, c->stream, user_queries(c), P->dev.d_off, P->dev.d_vals, P->dev.v0, lo, hi, nuq,
                           S.d_p_pack, S.d_p_stat);
    hipLaunchKernelGGL(hvs_k_in_scan, dim3(1), dim3(1024), 0, c->stream, S.d_p_pack, nuq, S.d_p_sub_off, S.d_p_eff, S.d_p_stat);
    HVS_HIP(c, hipGetLastError());
    HVS_HIP(c, hipEventRecord(S.ev_x1, c->stream));
    unsigned long long st[3] = {0, 0, 0};
    HVS_HIP(c, hipMemcpyAsync(st, S.d_p_stat, sizeof(st), hipMemcpyDeviceToHost, c->stream));
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, S.ev_x0, S.ev_x1);
    P->plan_ms = ms;
    if (st[0] & HVS_INP_MALFORMED) return fail(c, HVS_EINVAL, "hvs_set_category_sets_device: malformed offsets");
    if (st[0] & HVS_INP_TOO_MANY) return fail(c, HVS_EINVAL, "hvs_set_category_sets_device: a set of more than 64 distinct categories");
    if (st[1] >= 0xFFFFFFFFull) return fail(c, HVS_EINVAL, "hvs_set_category_sets_device: too many sub-queries");
    P->nsub = (uint32_t)st[1];
    P->dev.sub_if_all_c = st[2];
    P->sub_off.resize((size_t)nuq + 1u);
    P->eff.resize(nuq);
    HVS_HIP(c, hipMemcpyAsync(P->sub_off.data(), S.d_p_sub_off, P->sub_off.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (nuq) HVS_HIP(c, hipMemcpyAsync(P->eff.data(), S.d_p_eff, P->eff.size(), hipMemcpyDeviceToHost, c->stream));
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    return HVS_OK;
}

// The copies in_plan_device made of a CSR on another GPU are needed from the count to the fill only: the call that made them
// gives them back, whichever way it ends (the rest of the scratch, 9 bytes per user query, stays for the next attach).
int in_plan_release(hvs_ctx* c)
{
    HvsInSet& S = c->qs.in;
    if (!S.d_p_off && !S.d_p_vals) return HVS_OK;
    HVS_HIP(c, hipSetDevice(c->device));
    HvsRowSet::drop(S.d_p_off, S.d_p_vals);
    S.p_off_cap = S.pv_cap = 0;
    return HVS_OK;
}

// ---- the three clients' own steps (ExpandedKind::payload, expand, merge) and their descriptors ----
// category sets: a host plan's arrays are uploaded; of a plan made on the device, sub_off is copied and the fill kernel writes
// parent, value and the rebased offsets (part of expand_ms, as plan_ms is)
int sets_payload(hvs_ctx* c, const InPlan& P)
{
    HvsInSet& S = c->qs.in;
    if (P.dev.made) {
        if (hipMemcpyAsync(S.d_sub_off, S.d_p_sub_off, ((size_t)P.nuq + 1u) * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
            return fail(c, HVS_EHIP, "hvs_set_category_sets_device: the copy of the plan failed");
        return HVS_OK;
    }
    const InPlan::Host& H = P.host;
    auto up = [&](void* dst, const void* src, size_t bytes) { return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream) : hipSuccess; };
    if (up(S.d_sub_off, P.sub_off.data(), P.sub_off.size() * sizeof(uint32_t)) != hipSuccess ||
        up(S.d_set_off, H.set_off.data(), H.set_off.size() * sizeof(uint32_t)) != hipSuccess ||
        up(S.d_parent, H.parent.data(), H.parent.size() * sizeof(uint32_t)) != hipSuccess ||
        up(S.d_value, H.value.data(), H.value.size() * sizeof(float)) != hipSuccess)
        return fail(c, HVS_EHIP, "hvs_set_category_sets: upload of the plan failed");
    return HVS_OK;
}
dim3 expand_grid(uint32_t nsub) { return dim3((uint32_t)(((uint64_t)nsub * (HVS_QCOLS / 4u) + 255u) / 256u)); }  // (a thread per float4 of a row)
void sets_expand(hvs_ctx* c, const InPlan& P)
{
    const HvsInSet& S = c->qs.in;
    const InPlan::Device& V = P.dev;
    if (V.made && P.nuq)
        hipLaunchKernelGGL(hvs_k_in_fill, dim3((P.nuq + 3u) / 4u), dim3(256), 0, c->stream, S.d_uq, V.d_off, V.d_vals, V.v0, V.lo, P.nuq, S.d_sub_off, S.d_p_eff,
                           S.d_set_off, S.d_parent, S.d_value);
    if (P.nsub)
        hipLaunchKernelGGL(hvs_k_expand_in, expand_grid(P.nsub), dim3(256), 0, c->stream, reinterpret_cast<const float4*>(S.d_uq), S.d_parent, S.d_value,
                           S.d_set_off, P.nsub, reinterpret_cast<float4*>(c->d_q));
}
// extra vectors and extra clauses: the slice's extras -- `floats` of them from `src` -- into *buf; nothing else is uploaded,
// the fill kernels write sub_off and parent from the staged offsets
int extras_in(hvs_ctx* c, float** buf, size_t& cap, const float* src, int src_dev, size_t floats)
{
    const int rc = ensure_room(c, buf, cap, floats);
    return rc ? rc : copy_in(c, *buf, src, src_dev, floats * sizeof(float));
}
int vectors_payload(hvs_ctx* c, const InPlan& P)
{
    HvsInSet& S = c->qs.in;
    return extras_in(c, &S.d_vecs, S.vecs_cap, P.csr.vecs, P.csr.src_dev, ((size_t)P.nsub - P.nuq) * HVS_NDIM);
}
void vectors_expand(hvs_ctx* c, const InPlan& P)
{
    const HvsInSet& S = c->qs.in;
    hipLaunchKernelGGL(hvs_k_fill_vectors, dim3(hvs_ceil_div(P.nuq + 1u, 256u)), dim3(256), 0, c->stream, S.v_stage.d_words, P.nuq, S.d_sub_off, S.d_parent);
    if (P.nsub)
        hipLaunchKernelGGL(hvs_k_expand_vectors, expand_grid(P.nsub), dim3(256), 0, c->stream, reinterpret_cast<const float4*>(S.d_uq), S.d_parent, S.d_sub_off,
                           reinterpret_cast<const float4*>(S.d_vecs), P.nsub, reinterpret_cast<float4*>(c->d_q));
}
int clauses_payload(hvs_ctx* c, const InPlan& P)
{
    HvsInSet& S = c->qs.in;
    const size_t ncl = (size_t)P.nsub - P.nuq;
    const int rc = extras_in(c, &S.d_attrs, S.attrs_cap, P.csr.attrs, P.csr.src_dev, ncl * 4u);
    return rc || !P.csr.vecs ? rc : extras_in(c, &S.d_vecs, S.vecs_cap, P.csr.vecs, P.csr.src_dev, ncl * HVS_NDIM);
}
void clauses_expand(hvs_ctx* c, const InPlan& P)
{
    const HvsInSet& S = c->qs.in;
    hipLaunchKernelGGL(hvs_k_fill_clauses, dim3(hvs_ceil_div(P.nuq + 1u, 4u)), dim3(256), 0, c->stream, S.v_stage.d_words, P.nuq, S.d_sub_off, S.d_parent);
    if (P.nsub)
        hipLaunchKernelGGL(hvs_k_expand_clauses, expand_grid(P.nsub), dim3(256), 0, c->stream, reinterpret_cast<const float4*>(S.d_uq), S.d_parent, S.d_sub_off,
                           reinterpret_cast<const float4*>(S.d_attrs), P.csr.vecs ? reinterpret_cast<const float4*>(S.d_vecs) : nullptr, P.nsub,
                           reinterpret_cast<float4*>(c->d_q));
}
// The merge kernels are templates over <scalar order, capacity> with one signature.  The dispatch over the two compile-time
// constants is written here, once; a client's `pick(ST, CAPT)` names its kernel.  hvs_k_merge_vectors merges by id, and pads from
// the EXPANDED rows (a pad row's smallest distance); hvs_k_merge_clauses likewise, for up to 256 lists, under a threshold.
template <typename Pick>
MergeKernel merge_kernel(bool scalar_order, int cap, Pick pick)
{
    MergeKernel k = nullptr;
    with_cap(cap, [&](auto CAPT) { k = scalar_order ? pick(std::true_type{}, CAPT) : pick(std::false_type{}, CAPT); });
    return k;
}
#define HVS_MERGE_OF(kernel) \
    [](auto ST, auto CAPT) -> MergeKernel { return kernel<decltype(ST)::value, decltype(CAPT)::value>; }

static_assert(HVS_VEC_MAX_EXTRA_ == HVS_VECTORS_MAX_EXTRA && HVS_VECTORS_MAX_EXTRA + 1 <= 64, "a merge streams at most 64 sub-lists");
static_assert(HVS_CLAUSE_MAX_EXTRA_ == HVS_CLAUSES_MAX_EXTRA && HVS_CLAUSES_MAX_EXTRA + 1 == 256, "hvs_k_merge_clauses streams at most 256 sub-lists");
const ExpandedKind kCategorySets{
    HvsInSet::Sets, {"hvs_set_category_sets", "hvs_set_category_sets_device"}, {"set_offsets", "d_set_offsets"}, "hvs_query_in",
    ": malformed offsets, a set of more than 64 distinct categories, or too many sub-queries", "hvs_in_stats",
    false, 0u, {nullptr, nullptr, nullptr}, nullptr, nullptr, false,
    sets_payload, sets_expand, [](const InPlan&) { return true; },  // (the sub-queries' categories are distinct: so are their rows)
    [](bool order, int cap) { return merge_kernel(order, cap, HVS_MERGE_OF(hvs_k_merge_in)); }, true, 3u};
const ExpandedKind kQueryVectors{
    HvsInSet::Vectors, {"hvs_set_query_vectors", "hvs_set_query_vectors_device"}, {"vec_offsets", "d_offsets"}, "hvs_query_vectors",
    ": malformed offsets, more than HVS_VECTORS_MAX_EXTRA extra vectors on a query, or too many sub-queries", "hvs_vectors_stats",
    true, HVS_VEC_MAX_EXTRA_,
    {": vec_offsets[0] is not 0", ": vec_offsets are not ascending", ": a query has more than HVS_VECTORS_MAX_EXTRA extra vectors"},
    &InPlan::Staged::vecs, ": vecs is NULL", false,
    vectors_payload, vectors_expand, [](const InPlan&) { return false; },  // (a row comes back under every vector it is near to)
    [](bool order, int cap) { return merge_kernel(order, cap, HVS_MERGE_OF(hvs_k_merge_vectors)); }, false, 3u};
const ExpandedKind kQueryClauses{
    HvsInSet::Clauses, {"hvs_set_query_clauses", "hvs_set_query_clauses_device"}, {"clause_offsets", "d_offsets"}, "hvs_query_clauses",
    ": malformed offsets, more than HVS_CLAUSES_MAX_EXTRA extra clauses on a query, too many sub-queries, or clause_attrs is NULL", "hvs_clauses_stats",
    true, HVS_CLAUSE_MAX_EXTRA_,
    {": clause_offsets[0] is not 0", ": clause_offsets are not ascending", ": a query has more than HVS_CLAUSES_MAX_EXTRA extra clauses"},
    &InPlan::Staged::attrs, ": clause_attrs is NULL", true,
    clauses_payload, clauses_expand, [](const InPlan& P) { return !P.csr.vecs; },  // (predicate-only clauses give a row ONE key)
    [](bool order, int cap) { return merge_kernel(order, cap, HVS_MERGE_OF(hvs_k_merge_clauses)); }, false, 5u};

// A plan of client K is put in force on its GPU: the user's rows move aside, room is made for the sub-queries, what the
// client's kernels read reaches the device (K.payload), they run between the two events (K.expand), and the engines' set
// becomes the expanded one.  A failure half-way (no room) leaves the context without a client, and without resident queries
// if the query buffer itself could not grow.  On a replicated context the root then detaches every other GPU too
// (commit_everywhere_or_detach_all): a client is attached on all GPUs or on none.
int in_commit(hvs_ctx* c, const ExpandedKind& K, InPlan& P)
{
    HvsInSet& S = c->qs.in;
    const uint32_t nuq = P.nuq, nsub = P.nsub;
    int rc;
    HVS_HIP(c, hipSetDevice(c->device));  // (a multi-GPU commit runs on a thread of its own: every buffer below is this GPU's)
    // the user's rows: already aside when a client is replaced
    if (!S.active) {
        if (!S.d_sub_off || nuq > S.uq_cap) {
            S.uq_cap = 0;
            if ((rc = dev_alloc(c, &S.d_uq, (size_t)nuq * HVS_QCOLS)) || (rc = dev_alloc(c, &S.d_sub_off, (size_t)nuq + 1u)) ||
                (rc = dev_alloc(c, &S.d_set_off, (size_t)nuq + 1u)) || (rc = per_query_room(c, S.user, kCaps | kCursors, nuq)))
                return rc;
            S.uq_cap = nuq;
        }
        HVS_HIP(c, hipMemcpyAsync(S.d_uq, c->d_q, (size_t)nuq * HVS_QCOLS * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
        HVS_HIP(c, hipStreamSynchronize(c->stream));
        S.nuq = nuq;
    }
    // from here on the context changes
    auto lost = [&](int code) {
        expanded_changed(c, false);
        if (c->nq_cap < nuq) c->nq = 0;
        else if (hipMemcpy(c->d_q, S.d_uq, (size_t)nuq * HVS_QCOLS * sizeof(float), hipMemcpyDeviceToDevice) == hipSuccess) c->nq = nuq;
        else c->nq = 0;
        return code;
    };
    if ((rc = ensure_room(c, &S.d_parent, S.sub_cap, nsub, &S.d_value))) return lost(rc);
    if ((rc = ensure_queries(c, nsub))) return lost(rc);  // (the cursor arrays follow when cursors come: ensure_after)
    if ((rc = K.payload(c, P))) return lost(rc);
    (void)hipEventRecord(S.ev_x0, c->stream);
    K.expand(c, P);
    (void)hipEventRecord(S.ev_x1, c->stream);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)  // (the host arrays go with this scope)
        return lost(fail(c, HVS_EHIP, std::string(K.set_fn[0]) + ": the expansion failed"));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, S.ev_x0, S.ev_x1);
    S.expand_ms = (double)ms + P.plan_ms;
    S.h_sub_off.swap(P.sub_off);
    S.h_eff.swap(P.eff);
    c->nq = nsub;
    S.client = &K;
    S.one_key_per_row = K.one_key_per_row(P);
    expanded_changed(c, true);
    return HVS_OK;
}

// hvs_set_category_sets on one GPU
int in_attach(hvs_ctx* c, const uint32_t* off, const float* vals, uint32_t nuq)
{
    InPlan P;
    int rc = in_begin(c);
    if (!rc) rc = in_plan_host(c, off, vals, nuq, &P);
    return rc ? rc : in_commit(c, kCategorySets, P);
}

// hvs_vectors_check's and hvs_clauses_check's arithmetic
uint32_t vec_check_core(const uint32_t* off, uint32_t nq, uint32_t max_extra)
{
    if (!off || off[0] != 0u) return 0xFFFFFFFFu;
    for (uint32_t q = 0; q < nq; ++q)
        if (off[q + 1] < off[q] || off[q + 1] - off[q] > max_extra) return 0xFFFFFFFFu;
    const uint64_t nsub = (uint64_t)off[nq] + nq;
    return nsub >= 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)nsub;
}

// The plan of one GPU's slice of a staged client's CSR, first half: the slice's offsets -- `nuq` + 1 entries from host memory
// (src_dev < 0) or from GPU src_dev -- are staged in v_stage and checked there against K.limit (leaf_stage, with an event pair
// around the check; `first`: the slice is the head of the caller's array).  Good offsets come back to the host
// too (4 bytes per query): sub_off[q] = off[q] - off[0] + q, and hvs_query_resident maps query ranges to sub-query ranges there.
// Nothing that a query or a later call reads changes; the caller judges the flags of all GPUs before any commit.
int csr_stage(hvs_ctx* c, const ExpandedKind& K, const uint32_t* off, int src_dev, uint32_t nuq, bool first, InPlan* P)
{
    HvsInSet& S = c->qs.in;
    const size_t bytes = ((size_t)nuq + 1u) * sizeof(uint32_t);
    int rc = leaf_stage(c, S.v_stage, true, off, src_dev, nuq + 1u, [&](const HvsStage& st) {
        HVS_HIP(c, hipEventRecord(S.ev_x0, c->stream));
        if (int rc2 = check_offsets(c, st, nuq, first, K.limit)) return rc2;
        HVS_HIP(c, hipEventRecord(S.ev_x1, c->stream));
        return HVS_OK;
    });
    if (rc) return rc;
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, S.ev_x0, S.ev_x1);
    P->nuq = nuq;
    P->plan_ms = ms;
    if (S.v_stage.flags) return HVS_OK;
    std::vector<uint32_t> o((size_t)nuq + 1u);
    HVS_HIP(c, hipMemcpy(o.data(), S.v_stage.d_words, bytes, hipMemcpyDeviceToHost));
    P->sub_off.resize((size_t)nuq + 1u);
    P->eff.resize(nuq);
    for (uint32_t q = 0; q <= nuq; ++q) P->sub_off[q] = o[q] - o[0] + q;
    for (uint32_t q = 0; q < nuq; ++q) P->eff[q] = o[q + 1] > o[q] ? 1u : 0u;
    P->nsub = P->sub_off[nuq];
    return HVS_OK;
}

// hvs_query_resident under an expanded set: user queries [q0, q0 + nq) = sub-queries [sub_off[q0], sub_off[q0 + nq)), answered
// by the engines with padding off FOR THIS CALL (the user's setting is the merge's), their re-runs resolved (the call's one host
// synchronisation, as part_run has), then one launch of the client's merge into the merged rows q0 .. q0 + nq.
int in_run(hvs_ctx* c, uint32_t q0, uint32_t nq, float sample_proportion)
{
    HvsInSet& S = c->qs.in;
    const ExpandedKind& K = *S.client;
    if (!c->d_data) return fail(c, HVS_ESTATE, "no data set loaded (hvs_load_data / hvs_gen_data)");
    if ((uint64_t)q0 + nq > S.nuq) return fail(c, HVS_EINVAL, "query range outside the resident query set");
    HVS_HIP(c, hipSetDevice(c->device));
    int rc;
    if (nq == 0u) return run_queries(c, S.h_sub_off[q0], 0u, sample_proportion, NoHook{});  // (nothing to merge)
    if ((rc = ensure_room(c, &S.d_m_ids, S.m_cap, (size_t)S.nuq * c->k, &S.d_m_dists))) return rc;
    const uint32_t s0 = S.h_sub_off[q0], s1 = S.h_sub_off[q0 + nq];
    {
        struct PaddingOff {  // a per-call override: the sub-queries' lists are partial answers
            hvs_ctx* c;
            bool was;
            ~PaddingOff() { c->padding = was; }
        } off{c, c->padding};
        c->padding = false;
        if ((rc = run_queries(c, s0, s1 - s0, sample_proportion, NoHook{}))) return rc;
        if ((rc = resolve_overflow(c))) return rc;
    }
    HVS_HIP(c, hipMemsetAsync(S.d_stat, 0, K.stat_words * sizeof(unsigned long long), c->stream));
    HVS_HIP(c, hipEventRecord(S.ev_m0, c->stream));
    hipLaunchKernelGGL(K.merge(c->scalar_order, c->cap), dim3((nq + 3u) / 4u), dim3(256), 0, c->stream, S.d_sub_off, q0, nq, c->d_out_ids, c->d_out_dists,
                       c->d_data, c->n, K.merge_user_rows ? S.d_uq : c->d_q, c->padding ? 1 : 0, masked(c) ? c->rs.d_pad_ids : nullptr, S.d_m_ids,
                       S.d_m_dists, c->k, S.d_stat);
    HVS_HIP(c, hipGetLastError());
    HVS_HIP(c, hipEventRecord(S.ev_m1, c->stream));
    HVS_HIP(c, hipEventRecord(c->call.ev_q1, c->stream));  // (the merge belongs to the call's device time)
    c->call.timing.nq = nq;  // (the user's)
    S.call = true;
    S.call_client = S.client;
    S.call_sub = s1 - s0;
    S.call_set_queries = S.call_max_set = 0;
    for (uint32_t p = q0; p < q0 + nq; ++p) {
        S.call_set_queries += S.h_eff[p];
        S.call_max_set = std::max(S.call_max_set, S.h_sub_off[p + 1] - S.h_sub_off[p]);
    }
    return HVS_OK;
}

int leaf_run_resident(hvs_ctx* c, uint32_t q0, uint32_t nq, float sample_proportion)
{
    return c->qs.in.active ? in_run(c, q0, nq, sample_proportion) : run_queries(c, q0, nq, sample_proportion, NoHook{});
}

// the last call's merge on one GPU (it ran on an expanded set: S.call): the first `words` of its counters and its device time
int leaf_merge_stats(hvs_ctx* c, unsigned long long* v, uint32_t words, float* ms)
{
    const HvsInSet& S = c->qs.in;
    HVS_HIP(c, hipMemcpy(v, S.d_stat, words * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HVS_HIP(c, hipEventElapsedTime(ms, S.ev_m0, S.ev_m1));
    return HVS_OK;
}

// What the three clients' stats share on one GPU: the call is over, *out is zeroed, and, if the last call ran under client K,
// the figures every info struct has -- some under names of its own: the queries with extras, the most sub-queries of one
// query, the keys read -- are filled in.  `own(*out, v)` adds the client's other counters from the merge's words v.
template <typename Info, typename Own>
int leaf_client_stats(hvs_ctx* c, const ExpandedKind& K, Info* out, uint32_t Info::*queries, uint32_t Info::*most, uint64_t Info::*keys, Own own)
{
    int rc = call_required(c);
    if (rc) return rc;
    *out = Info{};
    const HvsInSet& S = c->qs.in;
    if (!S.call || S.call_client != &K) return HVS_OK;
    unsigned long long v[HvsInSet::kStatWordsMax] = {};
    float ms = 0.f;
    if ((rc = leaf_merge_stats(c, v, K.stat_words, &ms))) return rc;
    out->*queries = S.call_set_queries;
    out->sub_queries = S.call_sub;
    out->*most = S.call_max_set;
    out->underfull_queries = (uint32_t)v[0];
    out->*keys = v[1];
    out->expand_ms = S.expand_ms;
    out->merge_ms = ms;
    own(*out, v);
    return HVS_OK;
}
int leaf_in_stats(hvs_ctx* c, hvs_in_info* out)
{
    return leaf_client_stats(c, kCategorySets, out, &hvs_in_info::set_queries, &hvs_in_info::max_set, &hvs_in_info::merged_keys,
                             [](hvs_in_info&, const unsigned long long*) {});
}
int leaf_vectors_stats(hvs_ctx* c, hvs_vectors_info* out)
{
    return leaf_client_stats(c, kQueryVectors, out, &hvs_vectors_info::multi_queries, &hvs_vectors_info::max_vectors, &hvs_vectors_info::merged_keys,
                             [](hvs_vectors_info& o, const unsigned long long* v) { o.duplicate_keys = v[2]; });
}
int leaf_clauses_stats(hvs_ctx* c, hvs_clauses_info* out)
{
    return leaf_client_stats(c, kQueryClauses, out, &hvs_clauses_info::clause_queries, &hvs_clauses_info::max_clauses, &hvs_clauses_info::read_keys,
                             [](hvs_clauses_info& o, const unsigned long long* v) { o.duplicate_keys = v[2], o.bounded_keys = v[3], o.skipped_chunks = v[4]; });
}

// The vec_query-equivalent region with host buffers on both sides (reference src/test.cpp:82-88), pipelined:
//   copy-in stream   pinned slot <- caller's queries (host copy), H2D, 65536 queries per piece, one BATCH ahead
//   compute stream   the engine, batch by batch (each batch waits for its last piece's H2D)
//   copy-out stream  D2H of a finished batch's ids (+ distances) into pinned slots while the next batch computes;
//                    the calling thread drains the slots into the caller's arrays
// Buffers the caller pinned itself (hipHostMalloc / hipHostRegister) skip the staging copies.  Overflowed queries
// (rare) are re-run at the end and their rows fetched again.
// `sink` (HVS_GATHER_PEER): finished pieces do not leave for the host but for GPU `sink->ctx`'s result buffer, rows
// sink->row0 + ..., over xGMI (hipMemcpyPeerAsync on this GPU's copy-out stream, under the next batch's compute); the
// root downloads the gathered block once every GPU is done.  out_ids / out_dists are then unused.
struct PeerSink {
    hvs_ctx* ctx;
    uint32_t row0;
    bool want_dists;
};

// The rows of the queries a call answered a second time (HvsCallState::reruns, resolved) leave again: to the peer sink row by
// row, or to the caller's arrays.
int fetch_rerun_rows(hvs_ctx* c, const PeerSink* sink, uint32_t* out_ids, float* out_dists)
{
    std::vector<uint32_t> list;
    for (const auto& [d_list, len] : c->call.reruns()) {
        list.resize(list.size() + len);
        if (len) HVS_HIP(c, hipMemcpy(&list[list.size() - len], d_list, (size_t)len * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    const size_t cnt = list.size(), words = cnt * c->k, row_bytes = c->k * sizeof(uint32_t);
    if (!cnt) return HVS_OK;
    // The rows are packed on the device (the idle candidate workspace is the scratch), leave in ONE copy and are scattered here:
    // thousands of 400-byte copies cost ~10 us each.  Row by row all the same: to a peer sink, and without room for the packing.
    uint32_t* scratch = reinterpret_cast<uint32_t*>(c->fb.cand);
    const bool fits = scratch && 2u * words * sizeof(uint32_t) <= c->fb_cand_entries * sizeof(uint64_t);
    if (sink || !fits) {
        for (uint32_t qi : list) {
            const size_t src = (size_t)qi * c->k, dst = sink ? ((size_t)sink->row0 + qi) * c->k : src;
            if (sink) {
                HVS_HIP(c, hipMemcpyPeerAsync(sink->ctx->d_out_ids + dst, sink->ctx->device, c->d_out_ids + src, c->device, row_bytes, c->stream));
                if (sink->want_dists)
                    HVS_HIP(c, hipMemcpyPeerAsync(sink->ctx->d_out_dists + dst, sink->ctx->device, c->d_out_dists + src, c->device, row_bytes, c->stream));
            } else {
                HVS_HIP(c, hipMemcpyAsync(out_ids + dst, c->d_out_ids + src, row_bytes, hipMemcpyDeviceToHost, c->stream));
                if (out_dists) HVS_HIP(c, hipMemcpyAsync(out_dists + dst, c->d_out_dists + src, row_bytes, hipMemcpyDeviceToHost, c->stream));
            }
        }
        HVS_HIP(c, hipStreamSynchronize(c->stream));
        return HVS_OK;
    }
    uint32_t* d_list = scratch + 2u * words;  // (the list itself rides behind the rows when there is room)
    ScopedDevBufs tmp;
    if ((2u * words + cnt) * sizeof(uint32_t) > c->fb_cand_entries * sizeof(uint64_t)) HVS_HIP(c, tmp.alloc(&d_list, cnt));
    std::vector<uint32_t> packed(words * (out_dists ? 2u : 1u));
    HVS_HIP(c, hipMemcpyAsync(d_list, list.data(), cnt * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    const dim3 grid(hvs_ceil_div((uint32_t)words, 256u));
    hipLaunchKernelGGL(hvs_k_gather_rows, grid, dim3(256), 0, c->stream, d_list, (uint32_t)cnt, c->d_out_ids, c->k, scratch);
    if (out_dists)
        hipLaunchKernelGGL(hvs_k_gather_rows, grid, dim3(256), 0, c->stream, d_list, (uint32_t)cnt, reinterpret_cast<const uint32_t*>(c->d_out_dists),
                           c->k, scratch + words);
    HVS_HIP(c, hipMemcpyAsync(packed.data(), scratch, packed.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < cnt; ++i) {
        std::memcpy(out_ids + (size_t)list[i] * c->k, packed.data() + i * c->k, row_bytes);
        if (out_dists) std::memcpy(out_dists + (size_t)list[i] * c->k, packed.data() + words + i * c->k, row_bytes);
    }
    return HVS_OK;
}

// One hvs_query's side of HvsCopyPipe: where the call stands in its pieces of 65536 queries, and the hooks of run_queries, which
// runs the engine batch by batch on its own schedule.  Before the kernels of batch b are enqueued the compute stream is made to
// wait for the batch's queries (staged here if the previous batch's hook has not done so): a batch never starts before its input
// is on the device.  After they have been enqueued: batch b+1's queries are staged and sent, the results of everything BEFORE batch b
// are sent out and drained, and s_out is told to wait for batch b.  A batch's host work hides under its own compute.
struct PipeCall {
    static constexpr uint32_t SQ = HvsCopyPipe::kStageQ, R = HvsCopyPipe::kRing;
    hvs_ctx* c;
    HvsCopyPipe& P;       // c->pipe
    const float* q_rows;  // the caller's nq queries, and where their rows go: the caller's arrays or the peer sink
    uint32_t nq;
    uint32_t* out_ids;
    float* out_dists;
    const PeerSink* sink;
    bool in_pinned, out_pinned;  // the copies skip the slots
    HostTrace& tr;
    uint32_t in_next = 0;                   // input pieces enqueued so far
    uint32_t out_enq = 0, out_drained = 0;  // result pieces enqueued / drained (global numbering over the call)
    uint32_t staged_q = 0;  // queries [0, staged_q) are enqueued on the copy-in stream and the compute stream waits for them
    uint32_t npieces() const { return hvs_ceil_div(nq, SQ); }
    int stage_in_until(uint32_t p1)  // --- copy-in: pieces [in_next, p1) -> device
    {
        for (; in_next < p1; ++in_next) {
            const uint32_t q0 = in_next * SQ, m = std::min(SQ, nq - q0);
            const size_t bytes = (size_t)m * HVS_QCOLS * sizeof(float);
            float* dst = c->d_q + (size_t)q0 * HVS_QCOLS;
            const float* src = q_rows + (size_t)q0 * HVS_QCOLS;
            if (in_pinned)
                HVS_HIP(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, P.s_in));
            else if (int rc = P.stage_in(dst, src, bytes, in_next))
                return rc;
        }
        return HVS_OK;
    }
    int drain_one()  // --- copy-out of result pieces: D2H on s_out into slot piece % 4, drained before piece + 4 is sent
    {
        const uint32_t i = out_drained % R, q0 = out_drained * SQ, m = std::min(SQ, nq - q0);
        const size_t nb = (size_t)m * c->k * sizeof(uint32_t), at = (size_t)q0 * c->k;
        HVS_HIP(c, hipEventSynchronize(P.ev_out[i]));
        staging_copy(out_ids + at, P.h_out_ids[i], nb);
        if (out_dists) staging_copy(out_dists + at, P.h_out_dists[i], nb);
        ++out_drained;
        return HVS_OK;
    }
    int copy_out_until(uint32_t p1)
    {
        hipStream_t s_out = P.s_out;
        for (; out_enq < p1; ++out_enq) {
            const uint32_t q0 = out_enq * SQ, m = std::min(SQ, nq - q0);
            const size_t nb = (size_t)m * c->k * sizeof(uint32_t), at = (size_t)q0 * c->k;
            if (sink) {
                const size_t dst = ((size_t)sink->row0 + q0) * c->k;
                HVS_HIP(c, hipMemcpyPeerAsync(sink->ctx->d_out_ids + dst, sink->ctx->device, c->d_out_ids + at, c->device, nb, s_out));
                if (sink->want_dists)
                    HVS_HIP(c, hipMemcpyPeerAsync(sink->ctx->d_out_dists + dst, sink->ctx->device, c->d_out_dists + at, c->device, nb, s_out));
                continue;
            }
            if (out_pinned) {
                HVS_HIP(c, hipMemcpyAsync(out_ids + at, c->d_out_ids + at, nb, hipMemcpyDeviceToHost, s_out));
                if (out_dists) HVS_HIP(c, hipMemcpyAsync(out_dists + at, c->d_out_dists + at, nb, hipMemcpyDeviceToHost, s_out));
                continue;
            }
            if (out_enq - out_drained >= R)
                if (int rc = drain_one()) return rc;
            const uint32_t i = out_enq % R;
            HVS_HIP(c, hipMemcpyAsync(P.h_out_ids[i], c->d_out_ids + at, nb, hipMemcpyDeviceToHost, s_out));
            if (out_dists) HVS_HIP(c, hipMemcpyAsync(P.h_out_dists[i], c->d_out_dists + at, nb, hipMemcpyDeviceToHost, s_out));
            HVS_HIP(c, hipEventRecord(P.ev_out[i], s_out));
        }
        return HVS_OK;
    }
    int send_input(uint32_t upto_q, bool wait_here)
    {
        upto_q = std::min(nq, upto_q);
        if (upto_q <= staged_q) {
            // staged by the previous batch's hook, which made ITS lane's stream wait: this batch's stream waits itself
            if (wait_here && staged_q) HVS_HIP(c, hipStreamWaitEvent(c->stream, P.ev_stage, 0));
            return HVS_OK;
        }
        if (int rc = stage_in_until(std::min(npieces(), hvs_ceil_div(upto_q, SQ)))) return rc;
        HVS_HIP(c, hipEventRecord(P.ev_stage, P.s_in));
        if (wait_here) HVS_HIP(c, hipStreamWaitEvent(c->stream, P.ev_stage, 0));
        if (staged_q == 0u) tr.mark("in0");
        staged_q = std::min(nq, in_next * SQ);
        return HVS_OK;
    }
    int before(uint32_t off, uint32_t nqb) { return send_input(off + nqb, true); }  // --- the hooks of run_queries
    int after(uint32_t off, uint32_t nqb, uint32_t next_nqb)
    {
        int rc = next_nqb ? send_input(off + nqb + next_nqb, false) : HVS_OK;
        if (!rc) rc = copy_out_until(off / SQ);  // whole pieces of the batches before this one
        return rc ? rc : P.after_compute(c->stream, P.s_out);
    }
    int flush()  // --- behind the last batch: what is left goes out, and has arrived when this returns
    {
        int rc = copy_out_until(npieces());
        while (!rc && !out_pinned && out_drained < out_enq) rc = drain_one();
        tr.mark("drained");
        if (!rc) HVS_HIP(c, hipStreamSynchronize(P.s_out));
        return rc;
    }
};

// `max_d2` (hvs_query_within): the queries' distance caps, nq floats of host memory -- 4 bytes per query, sent whole before the
// pipeline starts.
int leaf_query(hvs_ctx* c, const float* q_rows, uint32_t nq, float sample_proportion, uint32_t* out_ids, float* out_dists,
               const PeerSink* sink = nullptr, const float* max_d2 = nullptr, const float* after_d = nullptr, const uint32_t* after_i = nullptr,
               const uint32_t* ex_off = nullptr, const uint32_t* ex_ids = nullptr)
{
    if (!c->d_data) return fail(c, HVS_ESTATE, "no data set loaded (hvs_load_data / hvs_gen_data)");
    if (nq == 0) return HVS_OK;
    if (!q_rows || (!out_ids && !sink)) return fail(c, HVS_EINVAL, "hvs_query: q_rows / out_ids is NULL");
    const auto t_host0 = std::chrono::steady_clock::now();
    HostTrace tr;
    int rc = leaf_begin_queries(c, nq);
    if (rc) return rc;
    tr.mark("begin");
    const bool in_pinned = host_pointer_is_pinned(q_rows);
    // (a peer sink behaves like a pinned destination: asynchronous copies straight from the result buffer, nothing to drain)
    const bool out_pinned = sink || (host_pointer_is_pinned(out_ids) && (!out_dists || host_pointer_is_pinned(out_dists)));
    if ((rc = c->pipe.size_for(c->k, out_dists != nullptr && !sink, in_pinned ? 0u : nq, out_pinned ? 0u : nq))) return rc;
    tr.mark("staging");
    c->nq = nq;
    if ((rc = attach_for_call(c, max_d2, after_d, after_i, nq, ex_off, ex_ids))) return rc;  // (hvs_query_after: 8 bytes per query, sent whole too; lists likewise)
    PipeCall call{c, c->pipe, q_rows, nq, out_ids, out_dists, sink, in_pinned, out_pinned, tr};
    tr.mark("pointers");
    if ((rc = run_queries(c, 0, nq, sample_proportion, call, true))) return rc;
    tr.mark("enqueued");
    if ((rc = call.flush())) return rc;
    tr.mark("s_out");
    // queries answered a second time: re-run now, their rows fetched again
    const bool had_ovf = c->call.pending;
    if ((rc = resolve_overflow(c))) return rc;
    tr.mark("resolved");
    if (had_ovf && (rc = fetch_rerun_rows(c, sink, out_ids, out_dists))) return rc;
    c->call.host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host0).count();
    tr.mark("done");
    tr.flush("hvs_query", nq);
    return HVS_OK;
}

int leaf_last_timing(hvs_ctx* c, hvs_timing* out)
{
    int rc = call_required(c);
    if (rc) return rc;
    HVS_HIP(c, hipEventSynchronize(c->call.ev_q1));
    float ms = 0.f;
    HVS_HIP(c, hipEventElapsedTime(&ms, c->call.ev_q0, c->call.ev_q1));
    c->call.timing.query_ms = ms;
    double k = 0.0;
    for (int i = 0; i < c->call.n_launch_events; ++i) {
        HVS_HIP(c, hipEventElapsedTime(&ms, c->call.ev_k[2 * i], c->call.ev_k[2 * i + 1]));
        k += ms;
    }
    c->call.timing.main_kernel_ms = k;
    c->call.timing.main_kernel_launches = (uint32_t)c->call.n_launch_events;
    unsigned long long h[3];
    if ((rc = call_counters(c, HVS_CNT_PAIRS, h))) return rc;
    c->call.timing.pairs = h[0];
    c->call.timing.scanned_pairs = h[1];
    c->call.timing.rescored_pairs = h[2];
    c->call.timing.host_ms = c->call.host_ms;
    *out = c->call.timing;
    return HVS_OK;
}

// ---- live-row mask ----
// Install `words` (ceil(n / 64) words, bits past n clear, n_live bits set: checked by the caller) as the context's mask.
// `del_ids` (host, ids < n): the new mask is the old one less these rows -- applied on the device by hvs_k_mask_delete
// instead of a whole-mask upload.
int leaf_apply_mask(hvs_ctx* c, const std::vector<uint64_t>& words, uint32_t n_live, const uint32_t* del_ids, uint32_t del_count)
{
    HvsRowSet& s = c->rs;
    int rc = begin_mutation(c);
    if (rc) return rc;
    const size_t bytes = words.size() * sizeof(uint64_t);
    if (!s.d_pad_ids && (rc = dev_alloc(c, &s.d_pad_ids, (size_t)HVS_KMAX))) return rc;
    if (!s.d_mask_stat) {
        if ((rc = dev_alloc(c, &s.d_mask_stat, (size_t)2))) return rc;
        HVS_HIP(c, hipMemsetAsync(s.d_mask_stat, 0, 2 * sizeof(unsigned long long), c->stream));
    }
    if (s.h_live.empty()) s.h_live = all_live_words(c->n);
    bool fresh = false;
    if (!s.d_live) {
        const size_t cap64 = std::max(words.size(), mask_words(s.n_cap));  // (room for the rows D has room for)
        if ((rc = dev_alloc(c, &s.d_live, cap64 * 2u))) return rc;
        s.live_cap = (uint32_t)cap64;
        fresh = true;
    }
    bool revived = false;
    for (size_t i = 0; i < words.size(); ++i) revived = revived || (words[i] & ~s.h_live[i]) != 0ull;
    if (del_ids) {
        if (fresh) HVS_HIP(c, hipMemcpyAsync(s.d_live, s.h_live.data(), bytes, hipMemcpyHostToDevice, c->stream));
        if ((rc = ensure_room(c, &s.d_mask_ids, s.mask_ids_cap, del_count))) return rc;
        HVS_HIP(c, hipMemcpyAsync(s.d_mask_ids, del_ids, (size_t)del_count * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(hvs_k_mask_delete, dim3(hvs_ceil_div(del_count, 256u)), dim3(256), 0, c->stream, s.d_mask_ids, del_count, s.d_live);
        HVS_HIP(c, hipGetLastError());
    } else {
        HVS_HIP(c, hipMemcpyAsync(s.d_live, words.data(), bytes, hipMemcpyHostToDevice, c->stream));
    }
    HVS_HIP(c, hipStreamSynchronize(c->stream));  // (the sources are the caller's)
    s.h_live = words;
    s.n_dead = c->n - n_live;
    if ((rc = row_set_changed(c, revived ? RowChange::MaskRevivedRows : RowChange::MaskLostRows))) return rc;
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    return HVS_OK;
}

int leaf_mask_stats(hvs_ctx* c, hvs_mask_info* out)
{
    int rc = leaf_sync(c);
    if (rc) return rc;
    out->n_live = c->n - c->rs.n_dead;
    out->n_dead = c->rs.n_dead;
    unsigned long long v[1] = {0};
    if (c->rs.d_mask_stat) HVS_HIP(c, hipMemcpy(v, c->rs.d_mask_stat, sizeof(v), hipMemcpyDeviceToHost));
    out->tiles_patched = v[0];
    if ((rc = call_counters(c, HVS_CNT_DEAD_SURVIVORS, v))) return rc;
    out->dead_survivors = v[0];
    return HVS_OK;
}

// ---- appended rows ----

// room for n_cap rows in D and in the device mask, contents kept; nothing a query sees changes
int leaf_reserve_rows(hvs_ctx* c, uint32_t n_cap)
{
    HvsRowSet& s = c->rs;
    if (!c->d_data) return fail(c, HVS_ESTATE, "no data set loaded (hvs_load_data / hvs_gen_data)");
    int rc = begin_mutation(c);
    if (rc) return rc;
    if (n_cap > s.n_cap) {
        // (shared row sets, DESIGN 3.18: every set gets words for the new rows first, so that a failure leaves all as it was)
        const bool restride = s.n_sets && !s.sets_part_rows && set_words_for(n_cap) > s.sets_words;
        if (restride && (rc = sets_restride_next(c, set_words_for(n_cap)))) return rc;
        if ((rc = grow_keep(c, &c->d_data, (size_t)n_cap * HVS_DCOLS, (size_t)c->n * HVS_DCOLS, "hvs_reserve_rows: moving D: "))) {
            HvsRowSet::drop(s.d_sets_next);
            return rc;
        }
        if (restride) sets_swap_next(c, s.n_sets, set_words_for(n_cap));
        s.n_cap = n_cap;
    }
    const size_t cap64 = mask_words(s.n_cap);
    if (s.d_live && cap64 > s.live_cap) {  // (u32 words on the device: two to a word)
        if ((rc = grow_keep(c, &s.d_live, cap64 * 2u, mask_words(c->n) * 2u, "hvs_reserve_rows: moving the mask: "))) return rc;
        s.live_cap = (uint32_t)cap64;
    }
    return HVS_OK;
}

// first half of an append: capacity for `count` more rows (geometric growth), so that the second half cannot run out of
// memory on one GPU of several
int leaf_append_prepare(hvs_ctx* c, uint32_t count)
{
    const uint32_t need = c->n + count;  // (no overflow: checked by the caller)
    uint32_t want = c->rs.n_cap;
    if (need > c->rs.n_cap) want = (uint32_t)std::min<uint64_t>(0xFFFFFFFFull, std::max<uint64_t>(need, (uint64_t)c->rs.n_cap + c->rs.n_cap / 2u));
    int rc = leaf_reserve_rows(c, want);
    if (rc == HVS_ENOMEM && want > need) {  // no room for the growth step: exactly what is needed
        (void)hipGetLastError();
        c->err.clear();
        rc = leaf_reserve_rows(c, need);
    }
    return rc;
}

// fold the tail and the stale rows into the index: the load's own index build over all rows (the mask is re-applied by
// build_tiles' patch)
int leaf_reindex(hvs_ctx* c, bool force)
{
    if (!c->d_data) return fail(c, HVS_ESTATE, "no data set loaded (hvs_load_data / hvs_gen_data)");
    if (!force && tail_rows(c) == 0u && c->rs.h_stale.empty()) return HVS_OK;
    int rc = begin_mutation(c);
    if (rc) return rc;
    c->rs.h_stale.clear();  // (the new index describes every row as it is now)
    // (the live-row counts run along positions: their buffers are sized by the index that goes)
    if ((rc = dev_alloc(c, &c->ord[0].lp, (size_t)0))) return rc;
    if ((rc = dev_alloc(c, &c->ord[1].lp, (size_t)0))) return rc;
    const double load_ms = c->load_ms;  // hvs_timing.load_ms stays the load's
    c->index_ms = 0.0;
    rc = index_data(c);
    c->load_ms = load_ms;
    if (rc) return rc;
    c->rs.reindexes += 1u;
    c->rs.reindex_ms = c->index_ms;
    return HVS_OK;
}

// The one rule by which an append or an update ends with an index build: the rows behind the index plus the stale rows have
// outgrown the limit, and an index may be built at all (there is one; or the rule of a load allows a first one)
int fold_if_over_limit(hvs_ctx* c)
{
    const bool can_index = c->have_order || ((c->n >= kIndexMinRows || is_filter_engine(c->engine)) && !c->index_too_large);
    if (can_index && (uint64_t)rows_behind_index(c) + c->rs.h_stale.size() > tail_limit_of(c)) return leaf_reindex(c, true);
    return HVS_OK;
}

// second half: the rows, the mask bits, n -- and the index when the tail has outgrown its limit
int leaf_append_commit(hvs_ctx* c, const float* rows, uint32_t count)
{
    HvsRowSet& s = c->rs;
    HVS_HIP(c, hipSetDevice(c->device));
    const uint32_t n_old = c->n, n_new = n_old + count;
    int rc = upload_rows(c, c->d_data + (size_t)n_old * HVS_DCOLS, rows, (size_t)count * HVS_DCOLS);
    if (rc) return rc;
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    if (!s.h_live.empty()) {  // a mask has been set: the new rows start live
        std::vector<uint64_t> words = s.h_live;
        words.resize(mask_words(n_new), 0ull);
        mask_set_range(words, n_old, n_new);
        if (s.d_live) {
            const size_t w0 = n_old >> 6;
            HVS_HIP(c, hipMemcpyAsync(reinterpret_cast<uint64_t*>(s.d_live) + w0, words.data() + w0, (words.size() - w0) * sizeof(uint64_t),
                                      hipMemcpyHostToDevice, c->stream));
            HVS_HIP(c, hipStreamSynchronize(c->stream));
        }
        s.h_live.swap(words);
    }
    c->n = n_new;
    if ((rc = row_set_changed(c, RowChange::RowsAppended))) return rc;
    return fold_if_over_limit(c);
}

int leaf_append_stats(hvs_ctx* c, hvs_append_info* out)
{
    int rc = leaf_sync(c);
    if (rc) return rc;
    *out = hvs_append_info{};
    out->n_indexed = c->n_indexed;
    out->n_tail = tail_rows(c);
    out->tail_limit = tail_limit_of(c);
    out->reindexes = c->rs.reindexes;
    out->reindex_ms = c->rs.reindex_ms;
    unsigned long long v[2];
    if ((rc = call_counters(c, HVS_CNT_TAIL_PAIRS, v))) return rc;
    out->tail_pairs = v[0];
    out->tail_admitted = v[1];
    return HVS_OK;
}

// ---- updated rows ----
// first half of an update: every device buffer the second half writes, so that it cannot run out of memory on one GPU of
// several.  `n_stale_new`: length of the stale list after the update.  Nothing a query sees changes.
int leaf_update_prepare(hvs_ctx* c, uint32_t count, uint32_t n_stale_new)
{
    int rc = begin_mutation(c);
    if (rc) return rc;
    if (count > c->rs.upd_cap) {
        c->rs.upd_cap = 0;
        if ((rc = dev_alloc(c, &c->rs.d_upd_rows, (size_t)count * HVS_DCOLS))) return rc;
        if ((rc = dev_alloc(c, &c->rs.d_upd_ids, (size_t)count))) return rc;
        if ((rc = dev_alloc(c, &c->rs.d_upd_from, (size_t)count))) return rc;
        c->rs.upd_cap = count;
    }
    if (n_stale_new <= c->rs.h_stale.size()) return HVS_OK;  // no row becomes stale
    // the masked kernels are about to run: the mask's own buffers (an all-live mask where none has been set)
    if (c->rs.h_live.empty() || !c->rs.d_live || !c->rs.d_pad_ids || !c->rs.d_mask_stat) {
        const std::vector<uint64_t> words = c->rs.h_live.empty() ? all_live_words(c->n) : c->rs.h_live;
        if ((rc = leaf_apply_mask(c, words, c->n - c->rs.n_dead, nullptr, 0u))) return rc;
    }
    if (n_stale_new > c->rs.stale_cap) {
        const uint32_t want = (uint32_t)std::min<uint64_t>(c->n_indexed, std::max<uint64_t>(n_stale_new, 2ull * c->rs.stale_cap));
        // (the list is kept: this call may end before its second half, e.g. for want of room on another GPU)
        if ((rc = grow_keep(c, &c->rs.d_stale_ids, (size_t)want, c->rs.h_stale.size(), "hvs_update_rows: moving the stale list: ", c->rs.h_stale.data()))) return rc;
        c->rs.stale_cap = want;
    }
    const size_t words2 = 4u * mask_words(c->n_indexed);  // two planes
    return ensure_room(c, &c->rs.d_ilive, c->rs.ilive_cap, words2);  // (only while no row is stale: n_indexed does not change while one is)
}

// second half: the rows (one staged H2D + hvs_k_scatter_rows), the stale list and what follows from it (index-validity mask,
// tombstones, the live-row counts along the orderings) -- and the index when tail + stale rows have outgrown the limit.
// `uids` / `from` (nu entries): every id once, with the staged row that holds its last contents.
int leaf_update_commit(hvs_ctx* c, const float* rows, uint32_t count, const uint32_t* uids, const uint32_t* from, uint32_t nu,
                       const std::vector<uint32_t>& stale_new)
{
    HVS_HIP(c, hipSetDevice(c->device));
    int rc = upload_rows(c, c->rs.d_upd_rows, rows, (size_t)count * HVS_DCOLS);
    if (rc) return rc;
    HVS_HIP(c, hipMemcpyAsync(c->rs.d_upd_ids, uids, (size_t)nu * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HVS_HIP(c, hipMemcpyAsync(c->rs.d_upd_from, from, (size_t)nu * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    const uint64_t nelem = (uint64_t)nu * HVS_DCOLS;
    hipLaunchKernelGGL(hvs_k_scatter_rows, dim3((uint32_t)((nelem + 255u) / 256u)), dim3(256), 0, c->stream, c->rs.d_upd_rows, c->rs.d_upd_ids,
                       c->rs.d_upd_from, nu, c->d_data);
    HVS_HIP(c, hipGetLastError());
    if (stale_new.size() > c->rs.h_stale.size()) {
        HVS_HIP(c, hipMemcpyAsync(c->rs.d_stale_ids, stale_new.data(), stale_new.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        c->rs.h_stale = stale_new;
        if ((rc = row_set_changed(c, RowChange::StaleGrew))) return rc;
    }
    HVS_HIP(c, hipStreamSynchronize(c->stream));  // (the sources are the caller's)
    // (without orderings no row is stale and an update never builds the first index: that is an append's or hvs_reindex's to do)
    return c->have_order ? fold_if_over_limit(c) : HVS_OK;
}

int leaf_update_stats(hvs_ctx* c, hvs_update_info* out)
{
    int rc = leaf_sync(c);
    if (rc) return rc;
    *out = hvs_update_info{};
    out->n_stale = (uint32_t)c->rs.h_stale.size();
    out->limit = tail_limit_of(c);
    unsigned long long v[3];
    if ((rc = call_counters(c, HVS_CNT_STALE_PAIRS, v))) return rc;
    out->stale_pairs = v[0];
    out->stale_admitted = v[1];
    out->stale_survivors = v[2];
    return HVS_OK;
}

// ---- row compaction ----
// source rows per gather launch and rows of the bounce buffer; HVS_COMPACT_CHUNK overrides, read per call (any value >= 1)
uint32_t compact_chunk() { return env_u32("HVS_COMPACT_CHUNK", 65536u, 1u, 0xFFFFFFFFu); }

int free_call_scratch(hvs_ctx* c)  // of hvs_compact / hvs_trim_rows
{
    (void)hipSetDevice(c->device);
    c->rs.free_call_buffers();
    return HVS_OK;
}

// first half of a compaction: the earlier call's re-runs (they belong to the mask and the ids they were asked under) and the
// two scratch buffers, so that the second half cannot run out of memory on one GPU of several.  Nothing a query sees changes.
int leaf_compact_prepare(hvs_ctx* c, uint32_t first_dead, uint32_t chunk)
{
    int rc = begin_mutation(c);
    if (rc) return rc;
    if (!c->rs.d_live) return fail(c, HVS_ESTATE, "internal: rows are dead and the device mask is missing");
    const uint32_t bounce_rows = std::min(chunk, c->n - first_dead);
    HVS_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->rs.d_cmp_bounce), (size_t)bounce_rows * HVS_DCOLS * sizeof(float)));
    HVS_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->rs.d_cmp_rank), (((size_t)c->n + 31u) / 32u) * sizeof(uint32_t)));
    if (c->rs.n_sets)  // (shared row sets, DESIGN 3.18: the bounce bitmap of one set)
        HVS_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->rs.d_cmp_sets), (size_t)c->rs.sets_words * sizeof(uint32_t)));
    return HVS_OK;
}

// second half: the move, chunk by chunk on the context's stream (hvs_k_compact_gather into the bounce buffer, then a
// device-to-device copy to the rows' place: destination <= source, so a chunk's copy may overwrite its own source rows,
// which the gather has read, and never a later chunk's), then the state of a fresh load of the live rows and its index.
// `rank` (host): live rows in front of every 32-row mask word, ceil(n / 32) entries.
int leaf_compact_commit(hvs_ctx* c, const std::vector<uint32_t>& rank, uint32_t n_live, uint32_t first_dead, uint32_t chunk)
{
    HVS_HIP(c, hipSetDevice(c->device));
    const uint32_t n = c->n;
    auto live_before = [&](uint32_t id) -> uint32_t {  // live rows with an id below `id` (id <= n)
        if (id == n) return n_live;
        return rank[id >> 5] + (uint32_t)__builtin_popcount(mask_half(c->rs.h_live[id >> 6], id >> 5) & ((1u << (id & 31u)) - 1u));
    };
    HVS_HIP(c, hipMemcpyAsync(c->rs.d_cmp_rank, rank.data(), rank.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    // The shared row sets are renumbered first, while the mask and the rank table describe the old numbering: set
    // by set the bits of the live rows are packed into the zeroed bounce bitmap and copied back over the set.
    for (uint32_t st = 0; st < c->rs.n_sets; ++st) {
        uint32_t* set = c->rs.d_sets + (size_t)st * c->rs.sets_words;
        const size_t bytes = (size_t)c->rs.sets_words * sizeof(uint32_t);
        HVS_HIP(c, hipMemsetAsync(c->rs.d_cmp_sets, 0, bytes, c->stream));
        hipLaunchKernelGGL(hvs_k_row_sets_compact, dim3(hvs_ceil_div((uint32_t)rank.size(), 256u)), dim3(256), 0, c->stream, set, c->rs.d_live,
                           c->rs.d_cmp_rank, (uint32_t)rank.size(), c->rs.d_cmp_sets, c->rs.sets_words);
        HVS_HIP(c, hipGetLastError());
        HVS_HIP(c, hipMemcpyAsync(set, c->rs.d_cmp_sets, bytes, hipMemcpyDeviceToDevice, c->stream));
    }
    // HVS_TRACE: the gathers' and the copies' device time apart (an event between the two of every chunk)
    std::vector<hipEvent_t> ev_mid;
    HVS_HIP(c, hipEventRecord(c->call.ev_q0, c->stream));
    uint32_t chunks = 0;
    for (uint64_t a64 = first_dead; a64 < n; a64 += chunk, ++chunks) {
        const uint32_t a = (uint32_t)a64, b = (uint32_t)std::min<uint64_t>(n, a64 + chunk);
        const uint32_t ra = live_before(a), rb = live_before(b);
        const uint32_t words = ((b - 1u) >> 5) - (a >> 5) + 1u;
        if (kTrace) {
            hipEvent_t e[2] = {nullptr, nullptr};
            if (hipEventCreate(&e[0]) == hipSuccess && hipEventCreate(&e[1]) == hipSuccess) (void)hipEventRecord(e[0], c->stream);
            ev_mid.push_back(e[0]);
            ev_mid.push_back(e[1]);
        }
        hipLaunchKernelGGL(hvs_k_compact_gather, dim3(hvs_ceil_div(words, 4u)), dim3(256), 0, c->stream,
                           reinterpret_cast<const uint2*>(c->d_data), c->rs.d_live, c->rs.d_cmp_rank, a, b, ra, c->rs.d_cmp_bounce);
        HVS_HIP(c, hipGetLastError());
        if (kTrace && ev_mid.back()) (void)hipEventRecord(ev_mid.back(), c->stream);
        if (rb > ra)
            HVS_HIP(c, hipMemcpyAsync(c->d_data + (size_t)ra * HVS_DCOLS, c->rs.d_cmp_bounce, (size_t)(rb - ra) * HVS_DCOLS * sizeof(float),
                                      hipMemcpyDeviceToDevice, c->stream));
    }
    HVS_HIP(c, hipEventRecord(c->call.ev_q1, c->stream));
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    float ms = 0.f;
    HVS_HIP(c, hipEventElapsedTime(&ms, c->call.ev_q0, c->call.ev_q1));
    if (kTrace) {
        double gather_ms = 0.0;
        for (size_t i = 0; i + 1u < ev_mid.size(); i += 2u) {
            float g = 0.f;
            if (ev_mid[i] && ev_mid[i + 1u] && hipEventElapsedTime(&g, ev_mid[i], ev_mid[i + 1u]) == hipSuccess) gather_ms += g;
        }
        for (hipEvent_t e : ev_mid)
            if (e) (void)hipEventDestroy(e);
        std::fprintf(stderr, "[hvs trace] hvs_compact n=%u live=%u chunks=%u: move %.3f ms, gathers %.3f ms, copies %.3f ms\n", n, n_live, chunks,
                     ms, gather_ms, ms - gather_ms);
    }
    free_call_scratch(c);
    c->rs.cstat.compactions += 1u;
    c->rs.cstat.n_before = n;
    c->rs.cstat.n_after = n_live;
    c->rs.cstat.first_moved = first_dead;
    c->rs.cstat.chunks = chunks;
    c->rs.cstat.rows_moved = (uint64_t)n_live - first_dead;  // (every id below the first dead one is live)
    c->rs.cstat.move_ms = ms;
    // from here on the state of a fresh load of the live rows, in the room D has (n_cap stays)
    c->n = n_live;
    int rc = reset_row_set(c);
    if (rc) return rc;
    // a compaction, unlike a load, keeps the data set's figures (reindexes, reindex_ms; cstat it has just bumped), starts the
    // count of patched tile entries over even where no tile build will, and leaves no earlier call's timing to ask for.
    // NOTE: a load does neither of the last two; whether that is meant is not recorded (hvs_mask_info.tiles_patched, hvs_last_timing)
    if (c->rs.d_mask_stat) HVS_HIP(c, hipMemsetAsync(c->rs.d_mask_stat, 0, 2 * sizeof(unsigned long long), c->stream));
    call_forgotten(c);
    c->qs.drop_results();  // (they hold old ids: hvs_set_after_from_results must not read them; queries, sets, caps and cursors stay)
    // one index over all rows -- or none, by the rule of a load (fewer than 4096 rows, or no room for one)
    if (c->n >= kIndexMinRows || is_filter_engine(c->engine)) return leaf_reindex(c, true);
    free_index(c);
    // (no leaf_reindex here to free the live-row counts along the orderings that have gone: the next index -- hvs_set_engine
    // builds one without coming through leaf_reindex -- may cover more rows than they have room for)
    if ((rc = dev_alloc(c, &c->ord[0].lp, (size_t)0))) return rc;
    return dev_alloc(c, &c->ord[1].lp, (size_t)0);
}

// hvs_trim_rows, first half: the smaller buffer; second half: the rows, and the swap
int leaf_trim_prepare(hvs_ctx* c)
{
    int rc = begin_mutation(c);
    if (rc) return rc;
    if (c->rs.n_cap == c->n) return HVS_OK;
    HVS_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->rs.d_trim), (size_t)c->n * HVS_DCOLS * sizeof(float)));
    if (c->rs.n_sets && !c->rs.sets_part_rows && set_words_for(c->n) < c->rs.sets_words)  // (the shared row sets shrink with D)
        return sets_restride_next(c, set_words_for(c->n));
    return HVS_OK;
}

int leaf_trim_commit(hvs_ctx* c)
{
    if (!c->rs.d_trim) return HVS_OK;
    HVS_HIP(c, hipSetDevice(c->device));
    HVS_HIP(c, hipMemcpyAsync(c->rs.d_trim, c->d_data, (size_t)c->n * HVS_DCOLS * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    (void)hipFree(c->d_data);
    c->d_data = c->rs.d_trim;
    c->rs.d_trim = nullptr;
    c->rs.n_cap = c->n;
    if (c->rs.d_sets_next) sets_swap_next(c, c->rs.n_sets, set_words_for(c->n));
    return HVS_OK;
}

// ---------------------------------------------------------------------------------------------
// multi-GPU root
// ---------------------------------------------------------------------------------------------
// contiguous, balanced range of part r of `world` (the first total % world parts get one more): sharding.shard_range
void shard_range(uint32_t total, uint32_t r, uint32_t world, uint32_t& a, uint32_t& b)
{
    const uint32_t base = total / world, rem = total % world;
    a = r * base + std::min(r, rem);
    b = a + base + (r < rem ? 1u : 0u);
}

// the resident queries of a multi-GPU root, cut into one range per leaf: the queries a leaf holds (replicated D) or owns (row parts)
void cut_queries(hvs_ctx* root, uint32_t nq)
{
    const uint32_t N = (uint32_t)root->kids.size();
    root->kid_q0.assign(N + 1u, 0u);
    for (uint32_t r = 0; r < N; ++r) shard_range(nq, r, N, root->kid_q0[r], root->kid_q0[r + 1]);
}

// CPUs of the NUMA node of a GPU: PCI bus id -> /sys/bus/pci/devices/<id>/numa_node -> /sys/devices/system/node/node<k>/cpulist
// (best effort: empty when the platform does not say)
std::vector<int> device_node_cpus(int device)
{
    std::vector<int> cpus;
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), device) != hipSuccess) {
        (void)hipGetLastError();
        return cpus;
    }
    for (char* p = bus; *p; ++p) *p = (char)std::tolower((unsigned char)*p);
    int node = -1;
    if (FILE* f = std::fopen((std::string("/sys/bus/pci/devices/") + bus + "/numa_node").c_str(), "r")) {
        if (std::fscanf(f, "%d", &node) != 1) node = -1;
        std::fclose(f);
    }
    if (node < 0) return cpus;
    if (FILE* f = std::fopen(("/sys/devices/system/node/node" + std::to_string(node) + "/cpulist").c_str(), "r")) {
        int a = 0, b = 0;
        for (;;) {  // "0-15,128-143"
            if (std::fscanf(f, "%d", &a) != 1) break;
            b = a;
            int ch = std::fgetc(f);
            if (ch == '-') {
                if (std::fscanf(f, "%d", &b) != 1) break;
                ch = std::fgetc(f);
            }
            for (int x = a; x <= b && x < CPU_SETSIZE; ++x) cpus.push_back(x);
            if (ch != ',') break;
        }
        std::fclose(f);
    }
    return cpus;
}

// the calling thread (one leaf's host thread: staging copies, launches) moves next to its GPU; helper threads it starts
// inherit the mask
void pin_to_node(const hvs_ctx* leaf)
{
    if (leaf->node_cpus.empty()) return;
    cpu_set_t set;
    CPU_ZERO(&set);
    for (int x : leaf->node_cpus) CPU_SET(x, &set);
    (void)sched_setaffinity(0, sizeof(set), &set);
}

// run fn(leaf index) on one host thread per leaf (the reference's vec_query owns its worker threads the same way,
// optimized_parallel.hpp:82-89, threading.hpp:100-141) and return the first failure
template <typename Fn>
int for_each_leaf(hvs_ctx* root, Fn fn)
{
    const size_t N = root->kids.size();
    std::vector<int> rcs(N, HVS_OK);
    if (N == 1) {
        rcs[0] = fn(0u);
    } else {
        std::vector<std::thread> th;
        th.reserve(N);
        for (size_t r = 0; r < N; ++r)
            th.emplace_back([&, r]() {
                pin_to_node(root->kids[r]);  // (threads of this call only: the caller's own thread keeps its affinity)
                rcs[r] = fn((uint32_t)r);
            });
        for (auto& t : th) t.join();
    }
    for (size_t r = 0; r < N; ++r)
        if (rcs[r] != HVS_OK) {
            root->err = "GPU " + std::to_string(root->kids[r]->device) + " (part " + std::to_string(r) + "): " + root->kids[r]->err;
            return rcs[r];
        }
    return HVS_OK;
}

// leaves that hold part of the resident range [q0, q0 + nq): fn(leaf, local q0, count, offset into the caller's range)
template <typename Fn>
int for_each_resident_part(hvs_ctx* root, uint32_t q0, uint32_t nq, Fn fn)
{
    if (root->kid_q0.size() != root->kids.size() + 1u || (uint64_t)q0 + nq > root->kid_q0.back())
        return fail(root, HVS_EINVAL, "query range outside the resident query set");
    return for_each_leaf(root, [&](uint32_t r) -> int {
        const uint32_t a = std::max(q0, root->kid_q0[r]), b = std::min(q0 + nq, root->kid_q0[r + 1]);
        if (a >= b) return HVS_OK;
        return fn(root->kids[r], a - root->kid_q0[r], b - a, a - q0);
    });
}

// fn(leaf) on the context itself or on every GPU of a multi-GPU one
template <typename Fn>
int on_every_leaf(hvs_ctx* c, Fn fn)
{
    if (c->kids.empty()) return fn(c);
    return for_each_leaf(c, [&](uint32_t r) { return fn(c->kids[r]); });
}

// Each leaf's share of an array with one entry per resident query, `nq` of them: fn(leaf, first entry, entries, row0).  On a
// replicated context the share is the leaf's range of the queries (kid_q0) and row0 = 0; on a row-partitioned one every part
// takes the whole array, and row0 is the part's first global row.  (No resident queries: every share is empty.)
template <typename Fn>
int for_each_share(hvs_ctx* c, uint32_t nq, Fn fn)
{
    if (c->kids.empty()) return fn(c, 0u, nq, 0u);
    const bool cut = c->kid_q0.size() == c->kids.size() + 1u;
    return for_each_leaf(c, [&](uint32_t r) -> int {
        if (c->partitioned) return fn(c->kids[r], 0u, nq, c->part_row0.size() > r ? c->part_row0[r] : 0u);
        return fn(c->kids[r], cut ? c->kid_q0[r] : 0u, cut ? c->kid_q0[r + 1] - c->kid_q0[r] : 0u, 0u);
    });
}
// the caller's caps or cursors (caller_values) to every leaf (hvs_set_max_dist2*, hvs_set_after*), or, f == nullptr, off every leaf
int attach_everywhere(hvs_ctx* c, PerQuery what, const float* f, const uint32_t* u, int src_dev, uint32_t nq)
{
    return for_each_share(c, nq, [&](hvs_ctx* k, uint32_t first, uint32_t m, uint32_t row0) {
        return leaf_attach(k, what, caller_values(f ? f + first : f, u ? u + first : u, src_dev), m, row0);
    });
}
// ---- the staged attach, root side ----
// A leaf's share of a per-query array or CSR of `nq` queries: its queries [q0, q0 + m) and its row window.  A replicated context
// cuts by the owner ranges; a row-partitioned one gives every part all of it and the part's rows (the last part's window is
// open-ended: an id behind the rows of today names a row that an append may bring).
struct Share {
    hvs_ctx* k;
    uint32_t q0, m, row0, n_rows;
};
std::vector<Share> shares_of(hvs_ctx* c, uint32_t nq)
{
    std::vector<Share> sh;
    if (c->kids.empty()) sh.push_back({c, 0u, nq, 0u, 0xFFFFFFFFu});
    const uint32_t N = (uint32_t)c->kids.size();
    const bool cut = c->kid_q0.size() == N + 1u;
    for (uint32_t r = 0; r < N; ++r) {
        if (c->partitioned) {
            const uint32_t row0 = c->part_row0.size() > r + 1u ? c->part_row0[r] : 0u;
            sh.push_back({c->kids[r], 0u, nq, row0, r + 1u == N ? 0xFFFFFFFFu - row0 : c->part_row0[r + 1] - row0});
        } else
            sh.push_back({c->kids[r], cut ? c->kid_q0[r] : 0u, cut ? c->kid_q0[r + 1] - c->kid_q0[r] : 0u, 0u, 0xFFFFFFFFu});
    }
    return sh;
}
template <typename F>  // f(share, its index) on every share, one host thread per GPU
int on_shares(hvs_ctx* c, const std::vector<Share>& sh, F f)
{
    if (c->kids.empty()) return f(sh[0], (size_t)0);
    return for_each_leaf(c, [&](uint32_t r) { return f(sh[r], (size_t)r); });
}
// Every share is staged (`stage(share, index)`: a leaf_stage into the area `area` names) and the root judges all GPUs' flags
// before any GPU commits: HVS_EINVAL, with the text `why` has for the first flag set, leaves every GPU as it was.
template <typename Stage>
int stage_and_judge(hvs_ctx* c, const std::vector<Share>& sh, const HvsStage& (*area)(const hvs_ctx*), const char* fn, const Refusal& why, Stage stage)
{
    if (int rc = on_shares(c, sh, stage)) {
        (void)hipGetLastError();  // (HIP's last error is the failed call's: the next call must not trip over it)
        return rc;
    }
    uint32_t flags = 0;
    for (const Share& s : sh) flags |= area(s.k).flags;
    if (!flags) return HVS_OK;
    return fail(c, HVS_EINVAL, std::string(fn) + (flags & HVS_OFF_BAD_FIRST ? why.bad_first : flags & HVS_OFF_BAD_ORDER ? why.bad_order : why.bad_long));
}
const HvsStage& off_stage_of(const hvs_ctx* k) { return k->qs.off_stage; }
const HvsStage& idx_stage_of(const hvs_ctx* k) { return k->qs.idx_stage; }
const HvsStage& v_stage_of(const hvs_ctx* k) { return k->qs.in.v_stage; }
// ... and every share commits; a failed commit (a copy or an allocation: some GPUs may hold the new values and some the old)
// leaves the attachment in force on none
template <typename Commit>
int commit_or_detach(hvs_ctx* c, const std::vector<Share>& sh, int attachment, Commit commit)
{
    const int rc = on_shares(c, sh, commit);
    if (rc)
        for (const Share& s : sh) s.k->qs.attached(attachment) = false;
    return rc;
}

// The caller's id lists of kind K (CSR: `nq` + 1 offsets, the ids; host memory, src_dev < 0, or device memory of GPU src_dev) to
// every leaf, or, `off` nullptr, off every leaf.  `first`: `off` is the head of the caller's array (a leaf of a replicated
// hvs_query_excluding gets a slice that the root has checked).
int lists_everywhere(hvs_ctx* c, const ListKind& K, const uint32_t* off, const uint32_t* ids, int src_dev, uint32_t nq, bool first, const char* fn)
{
    if (!off) return on_every_leaf(c, [&](hvs_ctx* k) { return leaf_detach_flag(k, K.flag); });
    const std::vector<Share> sh = shares_of(c, nq);
    const std::string name = std::string(": ") + K.offsets, not_zero = name + "[0] is not 0", not_ascending = name + " are not ascending";
    int rc = stage_and_judge(c, sh, off_stage_of, fn, Refusal{not_zero.c_str(), not_ascending.c_str(), K.too_long},
                             [&](const Share& s, size_t) { return leaf_lists_stage(s.k, K, off + s.q0, src_dev, s.m, first && s.q0 == 0u); });
    if (rc) return rc;
    if (!ids)
        for (const Share& s : sh)
            if (s.k->qs.off_stage.total()) return fail(c, HVS_EINVAL, std::string(fn) + ": the id array is NULL and the offsets name entries");
    return commit_or_detach(c, sh, K.flag, [&](const Share& s, size_t) { return leaf_lists_commit(s.k, K, ids, src_dev, s.m, s.row0, s.n_rows); });
}
// hvs_query_after / hvs_query_within / hvs_query_excluding: the call's caps, cursors and lists (host memory, `nq` each, the lists
// as a CSR whose offsets the caller has checked; nullptr: none) onto the queries just installed
int attach_for_call(hvs_ctx* c, const float* max_d2, const float* after_d, const uint32_t* after_i, uint32_t nq, const uint32_t* ex_off,
                    const uint32_t* ex_ids)
{
    int rc = max_d2 ? attach_everywhere(c, PerQuery::Caps, max_d2, nullptr, -1, nq) : HVS_OK;
    if (!rc && after_d) rc = attach_everywhere(c, PerQuery::Cursors, after_d, after_i, -1, nq);
    if (!rc && ex_off) rc = lists_everywhere(c, kExcludeLists, ex_off, ex_ids, -1, nq, false, "hvs_query_excluding");
    return rc;
}

// ---- the expanded set's clients, root side ----
// Every share commits its plan (`commit(share, index)`: an in_commit).  A failed commit on a replicated context (no room:
// in_commit left that GPU without a client) leaves no GPU under one: every GPU is detached, the context answers plain queries
// on every GPU whose query buffer survived, and the failing GPU's error is the call's.
template <typename Commit>
int commit_everywhere_or_detach_all(hvs_ctx* c, const std::vector<Share>& sh, Commit commit)
{
    const int rc = on_shares(c, sh, commit);
    if (rc && !c->kids.empty()) {
        const std::string err = c->err;
        for (hvs_ctx* k : c->kids) (void)in_detach(k);
        (void)hipGetLastError();
        c->err = err;
    }
    return rc;
}
// The setters of a staged client K (hvs_set_query_vectors*, hvs_set_query_clauses*) on every GPU: the CSR -- `off` and the
// extras `csr` -- from host memory (csr.src_dev < 0) or from GPU src_dev (checked and waited for by the caller).  A replicated
// context cuts it by the owner ranges.  Every GPU stages and checks its slice first and none changes unless every slice is
// good and the sub-queries of the whole context can be counted in 32 bits: HVS_EINVAL leaves every GPU as it was.
int expanded_everywhere(hvs_ctx* c, const ExpandedKind& K, const uint32_t* off, InPlan::Staged csr, uint32_t nq, const char* fn)
{
    const std::vector<Share> sh = shares_of(c, nq);
    std::vector<InPlan> plans(sh.size());
    int rc = stage_and_judge(c, sh, v_stage_of, fn, K.why, [&](const Share& s, size_t r) {
        return csr_stage(s.k, K, off + s.q0, csr.src_dev, s.m, s.q0 == 0u, &plans[r]);
    });
    if (rc) return rc;
    uint64_t total = 0;
    for (const Share& s : sh) total = std::max<uint64_t>(total, v_stage_of(s.k).end);  // (ascending offsets: the last slice's end)
    if (total + nq >= 0xFFFFFFFFull) return fail(c, HVS_EINVAL, std::string(fn) + ": too many sub-queries");
    if (total && !(csr.*K.required)) return fail(c, HVS_EINVAL, std::string(fn) + K.required_null);
    // (optional vectors without a single extra are no vectors whatever the pointer: every row has one key, cursors stay allowed)
    if (K.vecs_optional && total == 0u) csr.vecs = nullptr;
    return commit_everywhere_or_detach_all(c, sh, [&](const Share& s, size_t r) {
        const size_t first = v_stage_of(s.k).first;
        plans[r].csr = {csr.vecs ? csr.vecs + first * HVS_NDIM : nullptr, csr.attrs ? csr.attrs + first * 4u : nullptr, csr.src_dev};
        return in_commit(s.k, K, plans[r]);
    });
}

// the leaf whose row-set state speaks for the whole context (rows, mask and index are replicated)
const hvs_ctx* mask_leaf(const hvs_ctx* c) { return c->kids.empty() ? c : c->kids[0]; }
// ... for an entry point `fn` that needs a data set; nullptr (HVS_ESTATE, with the error text set) when there is none
const hvs_ctx* loaded_leaf(hvs_ctx* c, const char* fn)
{
    const hvs_ctx* L = mask_leaf(c);
    if (!L->d_data || !L->n) fail(c, HVS_ESTATE, std::string(fn) + ": no data set loaded");
    return L->d_data && L->n ? L : nullptr;
}

// A change in two halves: `prepare` secures on every GPU what `commit` needs before any GPU changes, so a failure so far
// leaves every context as it was.  `cleanup`, where there is one, frees the call's scratch on every GPU whichever way the
// call ends.  A failed call's error is taken off HIP's last-error slot.
template <typename Prepare, typename Commit>
int two_phase(hvs_ctx* c, Prepare prepare, Commit commit, int (*cleanup)(hvs_ctx*) = nullptr)
{
    int rc = on_every_leaf(c, prepare);
    if (!rc) rc = on_every_leaf(c, commit);
    if (cleanup) (void)on_every_leaf(c, cleanup);
    if (rc) (void)hipGetLastError();  // (HIP's last error is the failed call's: the next call must not trip over it)
    return rc;
}

// Figures of a multi-GPU context: leaf 0's view (rows, mask and index are replicated) plus, through `add(sum, leaf's)`, the
// other leaves' work counters of the last call, summed like hvs_timing's
template <typename Info, typename Add>
int leaf0_stats(hvs_ctx* c, Info* out, int (*leaf_stats)(hvs_ctx*, Info*), Add add)
{
    if (!c || !out) return HVS_EINVAL;
    if (c->kids.empty()) return leaf_stats(c, out);
    Info agg{};
    for (size_t r = 0; r < c->kids.size(); ++r) {
        Info m{};
        const int rc = leaf_stats(c->kids[r], &m);
        if (rc) return fail(c, rc, c->kids[r]->err);
        if (r == 0u) agg = m;
        else add(agg, m);
    }
    *out = agg;
    return HVS_OK;
}

// Per-call figures of a multi-GPU context: the leaves that took part in the last call, combined by `add(sum, leaf's)`.  On a
// row-partitioned context every part answered all the queries: `partitioned(sum)`, where given, puts the call's own figures
// in the place of the sums that would count a query once per part.
template <typename Info, typename Add>
int call_stats(hvs_ctx* c, Info* out, int (*leaf_stats)(hvs_ctx*, Info*), Add add, const std::function<void(Info&)>& partitioned = nullptr)
{
    if (!c || !out) return HVS_EINVAL;
    if (c->kids.empty()) return leaf_stats(c, out);
    if (c->partitioned && !c->part_timing_valid) return fail(c, HVS_ESTATE, "no query has run yet");
    Info agg{};
    bool any = c->partitioned;
    for (hvs_ctx* k : c->kids) {
        if (!k->call.valid) continue;  // (took no part in the last call)
        Info m{};
        const int rc = leaf_stats(k, &m);
        if (rc) return fail(c, rc, k->err);
        add(agg, m);
        any = true;
    }
    if (!any) return fail(c, HVS_ESTATE, "no query has run yet");
    if (c->partitioned && partitioned) partitioned(agg);
    *out = agg;
    return HVS_OK;
}

// ---------------------------------------------------------------------------------------------
// row-partitioned root (hvs_create_partitioned; include/hvs.h "row-partitioned context")
// ---------------------------------------------------------------------------------------------
#define HVS_NOT_PARTITIONED(c, fn) \
    if ((c)->partitioned) return fail((c), HVS_ESTATE, fn ": not supported on a row-partitioned context")

uint32_t part_tail_rows(const hvs_ctx* root) { return std::min(root->part_n, kPartTailRows); }

// gather and merge buffers of part r as the owner of `own` resident queries
int part_ensure_buffers(hvs_ctx* root, uint32_t r, uint32_t own)
{
    hvs_ctx* k = root->kids[r];
    HvsPart& P = k->part;
    const size_t need_m = (size_t)own * root->k, need_gx = need_m * (root->kids.size() - 1u);
    int rc;
    if ((rc = ensure_room(k, &P.d_m_ids, P.m_cap, need_m, &P.d_m_dists))) return rc;
    return ensure_room(k, &P.d_gx_ids, P.gx_cap, need_gx, &P.d_gx_dists);
}

// the plan of a data set of n rows in the root's books (no call has run on it yet)
void part_set_plan(hvs_ctx* root, uint32_t n)
{
    const uint32_t N = (uint32_t)root->kids.size();
    root->part_n = n;
    root->part_row0.assign(N + 1u, 0u);
    for (uint32_t r = 0; r < N && n; ++r) shard_range(n, r, N, root->part_row0[r], root->part_row0[r + 1]);
    root->pinfo = hvs_partition_info{};
    root->pinfo.n_parts = N;
    std::copy(root->part_row0.begin(), root->part_row0.end(), root->pinfo.row0);
    root->part_timing_valid = false;
}

// after a failure: nothing of this call is left running on any part (best effort)
void part_quiesce(hvs_ctx* root)
{
    for (hvs_ctx* k : root->kids) {
        (void)hipSetDevice(k->device);
        if (k->stream) (void)hipStreamSynchronize(k->stream);
        if (k->spare.stream) (void)hipStreamSynchronize(k->spare.stream);
    }
    (void)hipGetLastError();
}

// Resident queries [q0, q0 + nq) on every part's rows, then exchange and merge by owner.  Blocks until the merged answers exist.
int part_run(hvs_ctx* c, uint32_t q0, uint32_t nq, float sample_proportion)
{
    const uint32_t N = (uint32_t)c->kids.size(), K = c->k;
    if (!c->part_n) return fail(c, HVS_ESTATE, "no data set loaded (hvs_load_data / hvs_gen_data)");
    if (c->kid_q0.size() != N + 1u || (uint64_t)q0 + nq > c->kid_q0.back())
        return fail(c, HVS_EINVAL, "query range outside the resident query set");
    c->part_timing_valid = false;
    c->qs.call_capped = capped(c->kids[0]);  // (every part holds all the caps, or none does)
    c->qs.call_after = has_after(c->kids[0]);  // (likewise the cursors)
    c->qs.excl.call = has_excl(c->kids[0]);    // (and the lists)
    c->qs.call_rset = has_rset(c->kids[0]);    // (and the set indices)
    c->qs.cand.call = has_cand(c->kids[0]);
    if (nq == 0u) return HVS_OK;
    uint32_t local_sn[16];
    if (hvs_partition_plan(c->part_n, N, K, sample_proportion, nullptr, nullptr, local_sn)) return fail(c, HVS_EINVAL, "partition plan");
    // every part answers all the queries on its rows (its overflow re-runs included): the call's one synchronisation
    int rc = for_each_leaf(c, [&](uint32_t r) -> int {
        hvs_ctx* k = c->kids[r];
        HVS_HIP(k, hipSetDevice(k->device));
        int r2 = part_ensure_buffers(c, r, c->kid_q0[r + 1] - c->kid_q0[r]);
        if (r2) return r2;
        if (local_sn[r] == 0u) {  // nothing of the sampled prefix in this part: empty lists, no launch
            call_forgotten(k);
            HVS_HIP(k, hipMemsetAsync(k->d_out_ids + (size_t)q0 * K, 0xFF, (size_t)nq * K * sizeof(uint32_t), k->stream));
            HVS_HIP(k, hipStreamSynchronize(k->stream));
            return HVS_OK;
        }
        if ((r2 = run_queries_cut(k, q0, nq, cut_rows(k, local_sn[r]), NoHook{}))) return r2;
        return leaf_sync(k);
    });
    // owner r: the other parts' rows of its queries into its gather buffer, its own rows in place, one merge launch
    if (!rc)
        rc = for_each_leaf(c, [&](uint32_t r) -> int {
            hvs_ctx* k = c->kids[r];
            HvsPart& P = k->part;
            P.exchange_ms = P.merge_ms = 0.0;
            P.bytes = 0;
            P.padded = 0;
            const uint32_t a = std::max(q0, c->kid_q0[r]), b = std::min(q0 + nq, c->kid_q0[r + 1]);
            if (a >= b) return HVS_OK;
            const uint32_t own = c->kid_q0[r + 1] - c->kid_q0[r], lo = a - c->kid_q0[r], m = b - a;
            const size_t cnt = (size_t)m * K;
            HVS_HIP(k, hipSetDevice(k->device));
            HVS_HIP(k, hipMemsetAsync(P.d_padded, 0, sizeof(unsigned long long), k->stream));
            HVS_HIP(k, hipEventRecord(P.ev_x0, k->stream));
            HvsPartLists L{};
            uint32_t slot = 0;
            for (uint32_t p = 0; p < N; ++p) {
                L.row0[p] = c->part_row0[p];
                if (p == r) {
                    L.ids[p] = k->d_out_ids + (size_t)a * K;
                    L.dists[p] = k->d_out_dists + (size_t)a * K;
                    continue;
                }
                const hvs_ctx* src = c->kids[p];
                uint32_t* gi = P.d_gx_ids + ((size_t)slot * own + lo) * K;
                float* gd = P.d_gx_dists + ((size_t)slot * own + lo) * K;
                HVS_HIP(k, hipMemcpyPeerAsync(gi, k->device, src->d_out_ids + (size_t)a * K, src->device, cnt * sizeof(uint32_t), k->stream));
                HVS_HIP(k, hipMemcpyPeerAsync(gd, k->device, src->d_out_dists + (size_t)a * K, src->device, cnt * sizeof(float), k->stream));
                L.ids[p] = gi;
                L.dists[p] = gd;
                P.bytes += cnt * (sizeof(uint32_t) + sizeof(float));
                ++slot;
            }
            HVS_HIP(k, hipEventRecord(P.ev_x1, k->stream));
            const uint32_t tail_rows = part_tail_rows(c);
            with_cap(K <= 128u ? 256 : 512, [&](auto CAPT) {
                auto launch = [&](auto ST) {
                    hipLaunchKernelGGL((hvs_k_merge_parts<decltype(ST)::value, decltype(CAPT)::value>), dim3((m + 3u) / 4u), dim3(256), 0, k->stream, L, N,
                                       m, k->d_q + (size_t)a * HVS_QCOLS, P.d_tail, tail_rows, c->part_n, c->padding ? 1 : 0,
                                       P.d_m_ids + (size_t)lo * K, P.d_m_dists + (size_t)lo * K, K, P.d_padded);
                };
                if (c->scalar_order)
                    launch(std::true_type{});
                else
                    launch(std::false_type{});
            });
            HVS_HIP(k, hipGetLastError());
            HVS_HIP(k, hipEventRecord(P.ev_m1, k->stream));
            HVS_HIP(k, hipMemcpyAsync(&P.padded, P.d_padded, sizeof(unsigned long long), hipMemcpyDeviceToHost, k->stream));
            HVS_HIP(k, hipStreamSynchronize(k->stream));
            float ms = 0.f;
            HVS_HIP(k, hipEventElapsedTime(&ms, P.ev_x0, P.ev_x1));
            P.exchange_ms = ms;
            HVS_HIP(k, hipEventElapsedTime(&ms, P.ev_x1, P.ev_m1));
            P.merge_ms = ms;
            return HVS_OK;
        });
    if (rc) {
        part_quiesce(c);
        return rc;
    }
    hvs_partition_info& I = c->pinfo;
    I.padded_queries = 0;
    I.exchanged_bytes = 0;
    I.exchange_ms = I.merge_ms = 0.0;
    for (const hvs_ctx* k : c->kids) {
        I.padded_queries += (uint32_t)k->part.padded;
        I.exchanged_bytes += k->part.bytes;
        I.exchange_ms = std::max(I.exchange_ms, k->part.exchange_ms);
        I.merge_ms = std::max(I.merge_ms, k->part.merge_ms);
    }
    c->part_timing_valid = true;
    c->part_call_nq = nq;
    c->qs.answered(q0, nq, K, c->kids[0]->qs.set_gen);  // (the merged rows the resident set has, as run_queries_cut keeps them for one GPU)
    return HVS_OK;
}

// merged answers of resident queries [q0, q0 + nq), by owner range, to host memory
int part_download_results(hvs_ctx* c, uint32_t q0, uint32_t nq, uint32_t* out_ids, float* out_dists)
{
    const uint32_t K = c->k;
    for (size_t r = 0; r < c->kids.size() && c->kid_q0.size() == c->kids.size() + 1u; ++r) {
        const uint32_t a = std::max(q0, c->kid_q0[r]), b = std::min(q0 + nq, c->kid_q0[r + 1]);
        if (a < b && c->kids[r]->part.m_cap < (size_t)(c->kid_q0[r + 1] - c->kid_q0[r]) * K)
            return fail(c, HVS_ESTATE, "hvs_download_results: no results (hvs_query_resident has not run)");
    }
    return for_each_resident_part(c, q0, nq, [&](hvs_ctx* k, uint32_t lq0, uint32_t m, uint32_t off) -> int {
        HVS_HIP(k, hipSetDevice(k->device));
        HVS_HIP(k, hipMemcpyAsync(out_ids + (size_t)off * K, k->part.d_m_ids + (size_t)lq0 * K, (size_t)m * K * sizeof(uint32_t),
                                  hipMemcpyDeviceToHost, k->stream));
        if (out_dists)
            HVS_HIP(k, hipMemcpyAsync(out_dists + (size_t)off * K, k->part.d_m_dists + (size_t)lq0 * K, (size_t)m * K * sizeof(float),
                                      hipMemcpyDeviceToHost, k->stream));
        HVS_HIP(k, hipStreamSynchronize(k->stream));
        return HVS_OK;
    });
}

// the tail replica of every part after its rows are in place: from the caller's rows (host memory, or a device buffer of GPU
// src_dev >= 0), or generated
int part_fill_tail(hvs_ctx* root, hvs_ctx* k, const float* rows, int src_dev, uint64_t seed, int profile, uint32_t ncat)
{
    const uint32_t n = root->part_n, t = part_tail_rows(root);
    if (rows) {
        const float* last = rows + (size_t)(n - t) * HVS_DCOLS;
        const int rc = src_dev >= 0 ? copy_from_device(k, k->part.d_tail, last, src_dev, (size_t)t * HVS_DCOLS * sizeof(float))
                                    : upload_rows(k, k->part.d_tail, last, (size_t)t * HVS_DCOLS);
        if (rc) return rc;
    } else {
        hipLaunchKernelGGL(hvs_k_gen_data, dim3(hvs_ceil_div(t * HVS_DCOLS, 256u)), dim3(256), 0, k->stream, k->part.d_tail,
                           (uint64_t)t * HVS_DCOLS, seed, profile, ncat, (uint64_t)(n - t));
        HVS_HIP(k, hipGetLastError());
    }
    HVS_HIP(k, hipStreamSynchronize(k->stream));
    return HVS_OK;
}

// hvs_load_data (rows != nullptr) / hvs_load_data_device (rows in a device buffer of GPU src_dev >= 0) / hvs_gen_data of a
// partitioned context: part r takes ITS rows over its own link
int part_load(hvs_ctx* c, const float* rows, int src_dev, uint32_t n, uint64_t seed, int profile, uint32_t ncat)
{
    const uint32_t N = (uint32_t)c->kids.size();
    if (n / N < c->k) return fail(c, HVS_EINVAL, "row-partitioned context: every part needs at least k rows (n >= n_parts * k)");
    part_set_plan(c, n);
    const int rc = for_each_leaf(c, [&](uint32_t r) -> int {
        hvs_ctx* k = c->kids[r];
        const uint32_t a = c->part_row0[r], cnt = c->part_row0[r + 1] - a;
        const float* mine = rows ? rows + (size_t)a * HVS_DCOLS : nullptr;
        const int r2 = !rows ? leaf_gen_data(k, cnt, seed, profile, ncat, a)
                             : src_dev >= 0 ? leaf_load_data_device(k, mine, src_dev, cnt) : leaf_load_data(k, mine, cnt);
        return r2 ? r2 : part_fill_tail(c, k, rows, src_dev, seed, profile, ncat);
    });
    if (rc) {
        part_quiesce(c);
        c->part_n = 0;  // (parts may hold different data sets now: load again)
    }
    return rc;
}

// ---- what the entry points of caps, cursors, lists and the expanded set's clients share ----
// resident queries of the whole context
uint32_t resident_count(const hvs_ctx* c)
{
    if (c->kids.empty()) return user_nq(c);
    return c->kid_q0.size() == c->kids.size() + 1u ? c->kid_q0.back() : 0u;
}
// May cursors be attached?  Not while the expanded set's client (attached on every GPU or on none) lets a row come back under
// several keys -- extra vectors, or clauses with vectors of their own.  Under category sets and under
// predicate-only clauses a row has ONE key, and cursors go through leaf_attach.
bool cursors_refused(const hvs_ctx* c)
{
    const hvs_ctx* k = c->kids.empty() ? c : c->kids[0];
    return k->qs.in.active && !k->qs.in.one_key_per_row;
}
#define HVS_NO_CURSORS_ON_VECTORS(c, fn) \
    if (cursors_refused(c)) return fail((c), HVS_ESTATE, fn ": cursors do not compose with extra query vectors or clause vectors (a row would come back under another vector)")
// what the four entry points that attach per-query values check alike: `nq` is the number of resident queries ...
int check_resident_count(hvs_ctx* c, uint32_t nq, const char* fn)
{
    return nq == resident_count(c) ? HVS_OK : fail(c, HVS_EINVAL, std::string(fn) + ": nq is not the number of resident queries");
}
// ... and device buffers (`b`: a second one, or nullptr) are plain device memory of one GPU, *dev, on which the caller's work on
// `stream` is complete
int check_device_buffers(hvs_ctx* c, const void* a, const void* b, void* stream, const char* fn, int* dev)
{
    int dev2 = 0;
    int rc = device_of_buffer(c, a, fn, dev);
    if (!rc && b) rc = device_of_buffer(c, b, fn, &dev2);
    if (!rc && b && *dev != dev2) rc = fail(c, HVS_EINVAL, std::string(fn) + ": the two buffers are on different GPUs");
    return rc ? rc : wait_for_producer(c, *dev, stream);
}

// What the six setters of the expanded set's clients begin with (`device`: the _device form; `off`: the caller's offsets;
// `none`: every pointer of the caller's is NULL).  kAttach: go on and attach.  Anything else is the call's result: a refusal,
// or client K detached from every GPU -- no pointers, or no resident queries.
enum : int { kAttach = 1 };
int client_attach_begin(hvs_ctx* c, const ExpandedKind& K, bool device, const void* off, bool none, uint32_t nq)
{
    if (!c) return HVS_EINVAL;
    const std::string fn = K.set_fn[device];
    if (c->partitioned) return fail(c, HVS_ESTATE, fn + ": not supported (yet) on a row-partitioned context");
    auto detach = [&] { return on_every_leaf(c, [&](hvs_ctx* k) { return client_detach(k, K); }); };
    if (none) return detach();
    if (!loaded_leaf(c, fn.c_str())) return HVS_ESTATE;
    if (!off) return fail(c, HVS_EINVAL, fn + ": " + K.offsets[device] + " is NULL");
    if (int rc = check_resident_count(c, nq, fn.c_str())) return rc;
    return nq == 0u ? detach() : kAttach;
}
// The three one-shot calls (hvs_query_in, hvs_query_vectors, hvs_query_clauses).  `none`: every pointer of the CSR is NULL, a
// plain hvs_query; `good()`: the client's host check of the CSR, made before the resident set is replaced -- a refused call
// changes nothing; `set()`: the client's setter.  Then upload, set, run, download.
template <typename Good, typename Set>
int client_query(hvs_ctx* c, const ExpandedKind& K, bool none, const float* q_rows, uint32_t nq, float sample_proportion, uint32_t* out_ids, float* out_dists,
                 Good good, Set set)
{
    if (!c) return HVS_EINVAL;
    if (none) return hvs_query(c, q_rows, nq, sample_proportion, out_ids, out_dists);
    const std::string fn = K.query_fn;
    if (c->partitioned) return fail(c, HVS_ESTATE, fn + ": not supported (yet) on a row-partitioned context");
    if (!loaded_leaf(c, K.query_fn)) return HVS_ESTATE;
    if (nq == 0u) return HVS_OK;
    if (!q_rows || !out_ids) return fail(c, HVS_EINVAL, fn + ": q_rows / out_ids is NULL");
    if (!good()) return fail(c, HVS_EINVAL, fn + K.bad_query);
    int rc = hvs_upload_queries(c, q_rows, nq);
    if (!rc) rc = set();
    if (!rc) rc = hvs_query_resident(c, 0u, nq, sample_proportion);
    if (!rc) rc = hvs_download_results(c, 0u, nq, out_ids, out_dists);
    return rc;
}
// ... of a staged client: the offsets hold, and extras bring the array they cannot do without
bool csr_good(const ExpandedKind& K, const uint32_t* off, const InPlan::Staged& csr, uint32_t nq)
{
    const uint32_t nsub = vec_check_core(off, nq, K.limit);
    return nsub != 0xFFFFFFFFu && (nsub == nq || csr.*K.required);
}
// The three stats calls: refused on a row-partitioned context, else the leaves' figures combined by `add`
template <typename Info, typename Add>
int client_stats(hvs_ctx* c, const ExpandedKind& K, Info* out, int (*leaf_stats)(hvs_ctx*, Info*), Add add)
{
    if (c && out && c->partitioned) return fail(c, HVS_ESTATE, std::string(K.stats_fn) + ": not supported (yet) on a row-partitioned context");
    return call_stats<Info>(c, out, leaf_stats, add);
}

// What hvs_within_stats and hvs_after_stats start with on one GPU: the call is over, *out is zeroed, and, if the call ran with the
// feature (`on`), v holds its counters from slot `first` on
template <typename Info, size_t N>
int leaf_call_counters(hvs_ctx* c, Info* out, bool on, int first, unsigned long long (&v)[N])
{
    int rc = call_required(c);
    if (rc) return rc;
    *out = Info{};
    return on ? call_counters(c, first, v) : HVS_OK;
}
// ... and end with: under category sets the counted slots are the sub-lists', and a query is under-full when the merge found
// fewer than k keys
int in_underfull(hvs_ctx* c, uint32_t* underfull)
{
    if (!c->qs.in.call) return HVS_OK;
    unsigned long long v[HvsInSet::kStatWordsMin] = {};
    float ms = 0.f;
    const int rc = leaf_merge_stats(c, v, HvsInSet::kStatWordsMin, &ms);
    if (!rc) *underfull = (uint32_t)v[0];
    return rc;
}

int leaf_within_stats(hvs_ctx* c, hvs_within_info* out)
{
    unsigned long long v[2] = {0, 0};
    const int rc = leaf_call_counters(c, out, c->qs.call_capped, HVS_CNT_WITHIN_SLOTS, v);
    if (rc || !c->qs.call_capped) return rc;
    out->capped_queries = c->call.timing.nq;
    out->within_slots = v[0];
    out->underfull_queries = (uint32_t)v[1];
    return in_underfull(c, &out->underfull_queries);
}

int leaf_after_stats(hvs_ctx* c, hvs_after_info* out)
{
    unsigned long long v[3] = {0, 0, 0};
    const int rc = leaf_call_counters(c, out, c->qs.call_after, HVS_CNT_AFTER_SLOTS, v);
    if (rc || !c->qs.call_after) return rc;
    out->cursor_queries = c->call.timing.nq;
    out->after_slots = v[0];
    out->underfull_queries = (uint32_t)v[1];
    out->exhausted_queries = (uint32_t)v[2];  // (under category sets: counted per sub-query, as the slots are)
    return in_underfull(c, &out->underfull_queries);
}

int leaf_exclude_stats(hvs_ctx* c, hvs_exclude_info* out)
{
    unsigned long long v[3] = {0, 0, 0}, sink[1] = {0};
    int rc = leaf_call_counters(c, out, c->qs.excl.call, HVS_CNT_EXCL_SLOTS, v);
    if (rc || !c->qs.excl.call) return rc;
    if ((rc = call_counters(c, HVS_CNT_RERUN_SINK_EXCL_REFUSED, sink))) return rc;  // (the exact engine's re-runs count through the sink)
    out->excluding_queries = c->call.timing.nq;
    out->kept_slots = v[0];
    out->underfull_queries = (uint32_t)v[1];
    out->refused_keys = v[2] + sink[0];
    return in_underfull(c, &out->underfull_queries);
}

int leaf_candidates_stats(hvs_ctx* c, hvs_candidates_info* out)
{
    unsigned long long v[2] = {0, 0}, t[2] = {0, 0};
    int rc = leaf_call_counters(c, out, c->qs.cand.call, HVS_CNT_CAND_SLOTS, v);
    if (rc || !c->qs.cand.call) return rc;
    if ((rc = call_counters(c, HVS_CNT_PAIRS, t))) return rc;
    out->listed_queries = c->call.timing.nq;
    out->kept_slots = v[0];
    out->underfull_queries = (uint32_t)v[1];
    out->passing_ids = t[0];
    out->scanned_ids = t[1];
    for (int i = 0; i < c->call.n_launch_events; ++i) {  // (the scan's launches are the call's timed ones)
        float ms = 0.f;
        HVS_HIP(c, hipEventElapsedTime(&ms, c->call.ev_k[2 * i], c->call.ev_k[2 * i + 1]));
        out->scan_ms += ms;
    }
    return HVS_OK;
}

// ---- hvs_within_plan / hvs_after_plan: one row as the engines would leave it ----
// key order of the engines: distance bits (one NaN, above +inf), then id; equal keys keep their slots' order
struct PlanSlot {
    uint64_t key;
    uint32_t id;
    float dist;
};
PlanSlot plan_slot(float d, uint32_t id)
{
    uint32_t bits;
    std::memcpy(&bits, &d, sizeof(bits));
    if (d != d) {  // (the engines' keys carry one NaN)
        bits = 0x7FC00000u;
        std::memcpy(&d, &bits, sizeof(d));
    }
    return PlanSlot{((uint64_t)bits << 32) | id, id, d};
}
// the first k of the m slots (in key order, empty ones aside) that `keep` accepts, filled up to k with the pad rows or with empty
// slots, sorted; returns how many were kept
template <typename Keep>
uint32_t plan_row(const uint32_t* ids, const float* dists, uint32_t m, uint32_t k, Keep keep, const uint32_t* pad_ids, const float* pad_dists,
                  int padding, uint32_t* out_ids, float* out_dists)
{
    std::vector<PlanSlot> row;
    row.reserve(k);
    for (uint32_t j = 0; j < m && row.size() < k; ++j) {
        const PlanSlot s = plan_slot(dists[j], ids[j]);
        if (ids[j] != 0xFFFFFFFFu && keep(s)) row.push_back(s);
    }
    const uint32_t kept = (uint32_t)row.size();
    for (uint32_t s = 0; kept + s < k; ++s)
        row.push_back(padding && pad_ids && pad_dists ? plan_slot(pad_dists[s], pad_ids[s]) : PlanSlot{~0ull, 0xFFFFFFFFu, __builtin_inff()});
    std::stable_sort(row.begin(), row.end(), [](const PlanSlot& a, const PlanSlot& b) { return a.key < b.key; });
    for (uint32_t j = 0; j < k; ++j) {
        if (out_ids) out_ids[j] = row[j].id;
        if (out_dists) out_dists[j] = row[j].dist;
    }
    return kept;
}

}  // namespace

extern "C" {

const char* hvs_version(void) { return "hvs-mi355x 0.4 (gfx950)"; }

uint32_t hvs_plan_guess_m(uint32_t k, double seen_fraction, uint32_t pfail)
{
    return guess_m(seen_fraction, k, std::pow(10.0, -(double)pfail));
}

uint32_t hvs_plan_batches(uint32_t nq, int host_pipeline, uint32_t* out, uint32_t cap)
{
    const std::vector<uint32_t> sched = batch_schedule(nq, kBatchMfma, host_pipeline != 0);
    for (size_t i = 0; out && i < sched.size() && i < cap; ++i) out[i] = sched[i];
    return (uint32_t)sched.size();
}

const char* hvs_last_global_error(void) { return g_global_err.c_str(); }

int hvs_create(hvs_ctx** out, int device)
{
    if (!out) {
        g_global_err = "hvs_create: out is NULL";
        return HVS_EINVAL;
    }
    return leaf_create(out, device);
}

int hvs_create_on_devices(hvs_ctx** out, const int* devices, int n)
{
    if (!out || !devices || n < 1 || n > 64) {
        g_global_err = "hvs_create_on_devices: bad argument (1..64 device indices)";
        if (out) *out = nullptr;
        return HVS_EINVAL;
    }
    *out = nullptr;
    hvs_ctx* root = new (std::nothrow) hvs_ctx();
    if (!root) {
        g_global_err = "hvs_create_on_devices: out of host memory";
        return HVS_ENOMEM;
    }
    root->device = devices[0];
    for (int i = 0; i < n; ++i) {
        hvs_ctx* leaf = nullptr;
        const int rc = leaf_create(&leaf, devices[i]);
        if (rc != HVS_OK) {
            hvs_destroy(root);
            return rc;
        }
        if (n > 1 && env_u32("HVS_NUMA_PIN", 1u, 0u, 1u)) leaf->node_cpus = device_node_cpus(devices[i]);
        root->kids.push_back(leaf);
    }
    // peer access lets the replication of D and the peer gather use xGMI directly (best effort: without it the
    // runtime stages peer copies through host memory)
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
            if (devices[i] != devices[j]) {
                int can = 0;
                if (hipDeviceCanAccessPeer(&can, devices[i], devices[j]) == hipSuccess && can) {
                    (void)hipSetDevice(devices[i]);
                    (void)hipDeviceEnablePeerAccess(devices[j], 0);
                }
                (void)hipGetLastError();  // "already enabled" is fine
            }
    (void)hipSetDevice(devices[0]);
    *out = root;
    return HVS_OK;
}

int hvs_create_multi(hvs_ctx** out, int n_gpus)
{
    if (!out) {
        g_global_err = "hvs_create_multi: out is NULL";
        return HVS_EINVAL;
    }
    *out = nullptr;
    int count = 0;
    const hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0) {
        g_global_err = std::string("hvs_create_multi: no HIP device available (") + hipGetErrorString(e) +
                       "); this library has no CPU fallback";
        return HVS_EHIP;
    }
    if (n_gpus < 0 || n_gpus > count) {
        g_global_err = "hvs_create_multi: n_gpus outside 0..visible devices";
        return HVS_EINVAL;
    }
    if (n_gpus == 0) n_gpus = count;
    std::vector<int> devs(n_gpus);
    for (int i = 0; i < n_gpus; ++i) devs[i] = i;
    return hvs_create_on_devices(out, devs.data(), n_gpus);
}

int hvs_create_partitioned(hvs_ctx** out, const int* devices, int n_parts)
{
    if (!out || !devices || n_parts < 1 || n_parts > 16) {
        g_global_err = "hvs_create_partitioned: bad argument (1..16 device indices)";
        if (out) *out = nullptr;
        return HVS_EINVAL;
    }
    int rc = hvs_create_on_devices(out, devices, n_parts);
    if (rc) return rc;
    hvs_ctx* root = *out;
    root->partitioned = true;
    part_set_plan(root, 0u);
    for (hvs_ctx* k : root->kids) {
        k->padding = false;  // partial answers: the merge pads once, from the tail of the whole D
        HvsPart& P = k->part;
        hipError_t e = hipSetDevice(k->device);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&P.d_tail), (size_t)kPartTailRows * HVS_DCOLS * sizeof(float));
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&P.d_padded), sizeof(unsigned long long));
        for (hipEvent_t* ev : {&P.ev_x0, &P.ev_x1, &P.ev_m1})
            if (e == hipSuccess) e = hipEventCreate(ev);
        if (e != hipSuccess) {
            g_global_err = std::string("hvs_create_partitioned: ") + hipGetErrorString(e);
            hvs_destroy(root);
            *out = nullptr;
            return e == hipErrorOutOfMemory ? HVS_ENOMEM : HVS_EHIP;
        }
    }
    (void)hipSetDevice(devices[0]);
    return HVS_OK;
}

int hvs_partition_stats(hvs_ctx* c, hvs_partition_info* out)
{
    if (!c || !out) return HVS_EINVAL;
    if (!c->partitioned) return fail(c, HVS_ESTATE, "hvs_partition_stats: not a row-partitioned context");
    *out = c->pinfo;
    return HVS_OK;
}

int hvs_partition_plan(uint32_t n, uint32_t n_parts, uint32_t k, float sample_proportion, uint32_t* row0, uint32_t* sn, uint32_t* local_sn)
{
    if (n_parts < 1u || n_parts > 16u || n / n_parts < k) return HVS_EINVAL;
    const uint32_t s = sample_rows(sample_proportion, n);
    if (sn) *sn = s;
    for (uint32_t r = 0; r < n_parts; ++r) {
        uint32_t a, b;
        shard_range(n, r, n_parts, a, b);
        if (row0) row0[r] = a, row0[r + 1] = b;
        if (local_sn) local_sn[r] = std::min(std::max(s, a), b) - a;
    }
    return HVS_OK;
}

int hvs_num_gpus(const hvs_ctx* c) { return !c ? 0 : (c->kids.empty() ? 1 : (int)c->kids.size()); }

int hvs_device_count(void)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return count;
}

int hvs_set_gather(hvs_ctx* c, int mode)
{
    if (!c) return HVS_EINVAL;
    HVS_NOT_PARTITIONED(c, "hvs_set_gather");
    if (mode != HVS_GATHER_DIRECT && mode != HVS_GATHER_PEER) return fail(c, HVS_EINVAL, "hvs_set_gather: unknown mode");
    c->gather_mode = mode;
    return HVS_OK;
}

void hvs_destroy(hvs_ctx* c)
{
    if (!c) return;
    for (hvs_ctx* k : c->kids) hvs_destroy(k);
    if (c->kids.empty()) leaf_destroy(c);
    delete c;
}

const char* hvs_last_error(const hvs_ctx* c) { return c ? c->err.c_str() : "hvs: NULL context"; }

int hvs_set_engine(hvs_ctx* c, int engine)
{
    if (!c) return HVS_EINVAL;
    if (engine != HVS_ENGINE_AUTO && engine != HVS_ENGINE_EXACT_SCAN && !is_filter_engine(engine))
        return fail(c, HVS_EINVAL, "hvs_set_engine: unknown engine");
    c->engine = engine;
    if (!c->kids.empty()) return for_each_leaf(c, [&](uint32_t r) { return hvs_set_engine(c->kids[r], engine); });
    if (c->d_data && !c->have_order && (is_filter_engine(engine) || c->n >= kIndexMinRows)) {
        HVS_HIP(c, hipSetDevice(c->device));
        return build_index(c);
    }
    return HVS_OK;
}

int hvs_set_padding(hvs_ctx* c, int enabled)
{
    if (!c) return HVS_EINVAL;
    c->padding = enabled != 0;
    for (hvs_ctx* k : c->kids) k->padding = c->padding && !c->partitioned;  // (parts never pad: the merge does)
    return HVS_OK;
}

int hvs_set_distance_order(hvs_ctx* c, int order)
{
    if (!c) return HVS_EINVAL;
    if (order != HVS_ORDER_SIMD && order != HVS_ORDER_SCALAR) return fail(c, HVS_EINVAL, "hvs_set_distance_order: unknown order");
    c->scalar_order = order == HVS_ORDER_SCALAR;
    for (hvs_ctx* k : c->kids) k->scalar_order = c->scalar_order;
    return HVS_OK;
}

int hvs_set_k(hvs_ctx* c, uint32_t k)
{
    if (!c) return HVS_EINVAL;
    if (k < 8u || k > HVS_KMAX) return fail(c, HVS_EINVAL, "hvs_set_k: k outside 8..256 (the reference asserts KNN_LIMIT >= 8)");
    if (c->partitioned && c->part_n && c->part_n / (uint32_t)c->kids.size() < k)
        return fail(c, HVS_EINVAL, "hvs_set_k: a part of the row-partitioned data set has fewer than k rows");
    if (!c->kids.empty()) {
        const int rc = for_each_leaf(c, [&](uint32_t r) { return hvs_set_k(c->kids[r], k); });
        if (!rc) c->k = k;
        c->part_timing_valid = false;  // (result rows change size: nothing of the last call is left to report)
        return rc;
    }
    if (c->n && c->n - c->rs.n_dead < k) return fail(c, HVS_EINVAL, "hvs_set_k: the loaded data set has fewer than k (live) rows");
    if (k == c->k) return HVS_OK;
    int rc = begin_mutation(c);
    if (rc) return rc;
    c->k = k;
    c->cap = k <= 128u ? 256 : 512;
    // result rows change size: resident queries stay, their results do not; list workspaces are re-sized on demand
    const uint32_t had = k_changed(c);
    c->cand_lists = 0;
    c->rs.cut_valid = false;
    if ((rc = refresh_pad_ids(c))) return rc;
    return had ? ensure_results(c, had) : HVS_OK;
}

uint32_t hvs_get_k(const hvs_ctx* c) { return c ? c->k : 0u; }

uint32_t hvs_num_rows(const hvs_ctx* c) { return !c ? 0u : (c->partitioned ? c->part_n : c->kids.empty() ? c->n : c->kids[0]->n); }

int hvs_reserve(hvs_ctx* c, uint32_t nq)
{
    if (!c) return HVS_EINVAL;
    if (c->kids.empty()) return leaf_reserve(c, nq);
    const uint32_t N = (uint32_t)c->kids.size();
    if (c->partitioned)  // every part answers all nq queries and owns shard_range(nq, r, N) of them
        return for_each_leaf(c, [&](uint32_t r) -> int {
            const int rc = leaf_reserve(c->kids[r], nq);
            return rc ? rc : part_ensure_buffers(c, r, hvs_ceil_div(nq, N));
        });
    return for_each_leaf(c, [&](uint32_t r) { return leaf_reserve(c->kids[r], hvs_ceil_div(nq, N)); });
}

int hvs_load_data(hvs_ctx* c, const float* rows, uint32_t n)
{
    if (!c) return HVS_EINVAL;
    if (!rows) return fail(c, HVS_EINVAL, "hvs_load_data: rows is NULL");
    if (c->kids.empty()) return leaf_load_data(c, rows, n);
    if (c->partitioned) return part_load(c, rows, -1, n, 0u, 0, 0u);
    // D reaches the GPUs in two parallel phases: every GPU uploads ITS slice of the rows over its own PCIe link, then takes
    // the other slices from its peers over xGMI (each pair has its own link) -- an all-gather by peer copies -- and builds
    // its index.  (Round 2 uploaded everything to GPU 0 and let 7 peers pull 4 GB each from it after its index build;
    // HVS_LOAD_GATHER=0 keeps one upload + peer copies for A/B runs.)
    const uint32_t N = (uint32_t)c->kids.size();
    if (N == 1u || !env_u32("HVS_LOAD_GATHER", 1u, 0u, 1u)) {
        int rc = leaf_upload_data(c->kids[0], rows, n);
        if (rc) return fail(c, rc, c->kids[0]->err);
        return for_each_leaf(c, [&](uint32_t r) {
            if (r == 0u) {
                HVS_HIP(c->kids[0], hipSetDevice(c->kids[0]->device));
                return finish_data(c->kids[0]);
            }
            return leaf_load_data_from_peer(c->kids[r], c->kids[0]);
        });
    }
    std::vector<uint32_t> r0(N + 1u, 0u);
    for (uint32_t r = 0; r < N; ++r) shard_range(n, r, N, r0[r], r0[r + 1]);
    int rc = for_each_leaf(c, [&](uint32_t r) -> int {  // phase 1: own slice, host -> device
        hvs_ctx* k = c->kids[r];
        int r2 = begin_data(k, n);
        if (r2) return r2;
        HVS_HIP(k, hipEventRecord(k->call.ev_q0, k->stream));
        const size_t off = (size_t)r0[r] * HVS_DCOLS, cnt = (size_t)(r0[r + 1] - r0[r]) * HVS_DCOLS;
        if ((r2 = upload_rows(k, k->d_data + off, rows + off, cnt))) return r2;
        HVS_HIP(k, hipStreamSynchronize(k->stream));
        return HVS_OK;
    });
    if (rc) return rc;
    return for_each_leaf(c, [&](uint32_t r) -> int {  // phase 2: the other slices, device -> device; then the index
        hvs_ctx* k = c->kids[r];
        HVS_HIP(k, hipSetDevice(k->device));
        for (uint32_t step = 1; step < N; ++step) {  // (rank r starts with its right neighbour: the pairs of a step are disjoint)
            const uint32_t p = (r + step) % N;
            const size_t off = (size_t)r0[p] * HVS_DCOLS, cnt = (size_t)(r0[p + 1] - r0[p]) * HVS_DCOLS;
            if (cnt)
                HVS_HIP(k, hipMemcpyPeerAsync(k->d_data + off, k->device, c->kids[p]->d_data + off, c->kids[p]->device, cnt * sizeof(float),
                                              k->stream));
        }
        HVS_HIP(k, hipEventRecord(k->call.ev_q1, k->stream));
        HVS_HIP(k, hipStreamSynchronize(k->stream));
        k->n = n;
        return finish_data(k);
    });
}

// Every GPU takes the rows straight from the caller's buffer (a part of a partitioned context: its own rows and the tail
// replica): one copy per GPU over its own link to the source, no hop through a leaf that has them already.
int hvs_load_data_device(hvs_ctx* c, const float* d_rows, uint32_t n, void* stream)
{
    if (!c) return HVS_EINVAL;
    if (!d_rows) return fail(c, HVS_EINVAL, "hvs_load_data_device: d_rows is NULL");
    int dev = 0;
    int rc = device_of_buffer(c, d_rows, "hvs_load_data_device", &dev);
    if (!rc) rc = wait_for_producer(c, dev, stream);
    if (rc) return rc;
    if (c->kids.empty()) return leaf_load_data_device(c, d_rows, dev, n);
    if (c->partitioned) return part_load(c, d_rows, dev, n, 0u, 0, 0u);
    return for_each_leaf(c, [&](uint32_t r) { return leaf_load_data_device(c->kids[r], d_rows, dev, n); });
}

int hvs_gen_data(hvs_ctx* c, uint32_t n, uint64_t seed, int profile, uint32_t ncat)
{
    if (!c) return HVS_EINVAL;
    if (ncat == 0) return fail(c, HVS_EINVAL, "hvs_gen_data: ncat must be > 0");
    if (c->kids.empty()) return leaf_gen_data(c, n, seed, profile, ncat);
    if (c->partitioned) return part_load(c, nullptr, -1, n, seed, profile, ncat);
    return for_each_leaf(c, [&](uint32_t r) { return leaf_gen_data(c->kids[r], n, seed, profile, ncat); });
}

int hvs_download_data(hvs_ctx* c, uint32_t row0, uint32_t nrows, float* out_rows)
{
    if (!c) return HVS_EINVAL;
    if (c->partitioned) {
        if (!c->part_n) return fail(c, HVS_ESTATE, "no data set loaded");
        if (!out_rows || (uint64_t)row0 + nrows > c->part_n) return fail(c, HVS_EINVAL, "hvs_download_data: bad range");
        for (size_t r = 0; r < c->kids.size(); ++r) {  // the parts the range crosses
            const uint32_t a = std::max(row0, c->part_row0[r]), b = std::min(row0 + nrows, c->part_row0[r + 1]);
            if (a >= b) continue;
            const int rc = hvs_download_data(c->kids[r], a - c->part_row0[r], b - a, out_rows + (size_t)(a - row0) * HVS_DCOLS);
            if (rc) return fail(c, rc, c->kids[r]->err);
        }
        return HVS_OK;
    }
    if (!c->kids.empty()) {
        const int rc = hvs_download_data(c->kids[0], row0, nrows, out_rows);
        return rc ? fail(c, rc, c->kids[0]->err) : HVS_OK;
    }
    if (!c->d_data) return fail(c, HVS_ESTATE, "no data set loaded");
    if (!out_rows || (uint64_t)row0 + nrows > c->n) return fail(c, HVS_EINVAL, "hvs_download_data: bad range");
    HVS_HIP(c, hipSetDevice(c->device));
    HVS_HIP(c, hipMemcpyAsync(out_rows, c->d_data + (size_t)row0 * HVS_DCOLS, (size_t)nrows * HVS_DCOLS * sizeof(float),
                              hipMemcpyDeviceToHost, c->stream));
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    return HVS_OK;
}

int hvs_upload_queries(hvs_ctx* c, const float* q_rows, uint32_t nq)
{
    if (!c) return HVS_EINVAL;
    if (!q_rows && nq) return fail(c, HVS_EINVAL, "hvs_upload_queries: q_rows is NULL");
    if (c->kids.empty()) return leaf_upload_queries(c, q_rows, nq);
    if (c->partitioned) {  // all queries on every part; the ranges are the owners'
        cut_queries(c, nq);
        return for_each_leaf(c, [&](uint32_t r) { return leaf_upload_queries(c->kids[r], q_rows, nq); });
    }
    cut_queries(c, nq);
    return for_each_leaf(c, [&](uint32_t r) {
        return leaf_upload_queries(c->kids[r], q_rows + (size_t)c->kid_q0[r] * HVS_QCOLS, c->kid_q0[r + 1] - c->kid_q0[r]);
    });
}

int hvs_set_queries_device(hvs_ctx* c, const float* d_q_rows, uint32_t nq, void* stream)
{
    if (!c) return HVS_EINVAL;
    if (!d_q_rows && nq) return fail(c, HVS_EINVAL, "hvs_set_queries_device: d_q_rows is NULL");
    int dev = 0;
    if (nq) {  // (an empty set reads nothing)
        int rc = device_of_buffer(c, d_q_rows, "hvs_set_queries_device", &dev);
        if (!rc) rc = wait_for_producer(c, dev, stream);
        if (rc) return rc;
    }
    if (c->kids.empty()) return leaf_set_queries_device(c, d_q_rows, dev, nq);
    cut_queries(c, nq);
    if (c->partitioned)  // all queries on every part; the ranges are the owners'
        return for_each_leaf(c, [&](uint32_t r) { return leaf_set_queries_device(c->kids[r], d_q_rows, dev, nq); });
    return for_each_leaf(c, [&](uint32_t r) {
        return leaf_set_queries_device(c->kids[r], d_q_rows + (size_t)c->kid_q0[r] * HVS_QCOLS, dev, c->kid_q0[r + 1] - c->kid_q0[r]);
    });
}

void hvs_row_query(const float* row, int type, float dt, float* out_q)
{
    if (!row || !out_q) return;
    hvs_row_query_attrs(row[0], row[1], type, dt, out_q[0], out_q[1], out_q[2], out_q[3]);
    std::memcpy(out_q + 4, row + 2, (HVS_DCOLS - 2u) * sizeof(float));
}

int hvs_set_queries_from_rows(hvs_ctx* c, const uint32_t* ids, uint32_t first_id, uint32_t nq, int type, float dt)
{
    if (!c) return HVS_EINVAL;
    HVS_NOT_PARTITIONED(c, "hvs_set_queries_from_rows");
    if (type < HVS_ROWQ_KNN || type > HVS_ROWQ_BOTH) return fail(c, HVS_EINVAL, "hvs_set_queries_from_rows: type outside 0..3");
    if (!(dt >= 0.0f)) return fail(c, HVS_EINVAL, "hvs_set_queries_from_rows: dt is negative or NaN");
    const hvs_ctx* L = loaded_leaf(c, "hvs_set_queries_from_rows");
    if (!L) return HVS_ESTATE;
    if (!ids && (uint64_t)first_id + nq > L->n) return fail(c, HVS_EINVAL, "hvs_set_queries_from_rows: id outside [0, n)");
    const std::vector<uint64_t>& live = L->rs.h_live;  // (empty: no mask set, every row live)
    for (uint32_t i = 0; i < nq && (ids || !live.empty()); ++i) {
        const uint32_t id = ids ? ids[i] : first_id + i;
        if (id >= L->n) return fail(c, HVS_EINVAL, "hvs_set_queries_from_rows: id outside [0, n)");
        if (!live.empty() && !((live[id >> 6] >> (id & 63u)) & 1ull))
            return fail(c, HVS_EINVAL, "hvs_set_queries_from_rows: row " + std::to_string(id) + " is deleted");
    }
    if (c->kids.empty()) return leaf_set_queries_from_rows(c, ids, first_id, nq, type, dt);
    cut_queries(c, nq);
    return for_each_leaf(c, [&](uint32_t r) {  // each leaf builds its slice from its replica
        const uint32_t a = c->kid_q0[r];
        return leaf_set_queries_from_rows(c->kids[r], ids ? ids + a : nullptr, first_id + a, c->kid_q0[r + 1] - a, type, dt);
    });
}

int hvs_gen_queries(hvs_ctx* c, uint32_t nq, uint64_t seed, int profile, uint32_t ncat, int force_type,
                    uint64_t first_row)
{
    if (!c) return HVS_EINVAL;
    if (ncat == 0 || force_type > 3) return fail(c, HVS_EINVAL, "hvs_gen_queries: bad ncat / force_type");
    if (c->kids.empty()) return leaf_gen_queries(c, nq, seed, profile, ncat, force_type, first_row);
    if (c->partitioned) {
        cut_queries(c, nq);
        return for_each_leaf(c, [&](uint32_t r) { return leaf_gen_queries(c->kids[r], nq, seed, profile, ncat, force_type, first_row); });
    }
    cut_queries(c, nq);
    return for_each_leaf(c, [&](uint32_t r) {
        return leaf_gen_queries(c->kids[r], c->kid_q0[r + 1] - c->kid_q0[r], seed, profile, ncat, force_type, first_row + c->kid_q0[r]);
    });
}

int hvs_download_queries(hvs_ctx* c, uint32_t q0, uint32_t nq, float* out_rows)
{
    if (!c) return HVS_EINVAL;
    if (c->partitioned) {  // (every part holds them all)
        const int rc = hvs_download_queries(c->kids[0], q0, nq, out_rows);
        return rc ? fail(c, rc, c->kids[0]->err) : HVS_OK;
    }
    if (!c->kids.empty())
        return for_each_resident_part(c, q0, nq, [&](hvs_ctx* k, uint32_t lq0, uint32_t m, uint32_t off) {
            return hvs_download_queries(k, lq0, m, out_rows + (size_t)off * HVS_QCOLS);
        });
    if (!out_rows || (uint64_t)q0 + nq > user_nq(c)) return fail(c, HVS_EINVAL, "hvs_download_queries: bad range");
    HVS_HIP(c, hipSetDevice(c->device));
    HVS_HIP(c, hipMemcpyAsync(out_rows, user_queries(c) + (size_t)q0 * HVS_QCOLS, (size_t)nq * HVS_QCOLS * sizeof(float),
                              hipMemcpyDeviceToHost, c->stream));
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    return HVS_OK;
}

int hvs_query_resident(hvs_ctx* c, uint32_t q0, uint32_t nq, float sample_proportion)
{
    if (!c) return HVS_EINVAL;
    if (c->partitioned) return part_run(c, q0, nq, sample_proportion);
    if (!c->kids.empty()) {
        if (c->kid_q0.size() != c->kids.size() + 1u || (uint64_t)q0 + nq > c->kid_q0.back())
            return fail(c, HVS_EINVAL, "query range outside the resident query set");
        if (nq == 0u) return HVS_OK;
        // a GPU that holds none of the range's queries takes no part in this call: what it counted for an earlier call is not
        // this call's (call_stats sums the leaves whose call is valid), as in hvs_query for a GPU that got no queries
        return for_each_leaf(c, [&](uint32_t r) -> int {
            hvs_ctx* k = c->kids[r];
            const uint32_t a = std::max(q0, c->kid_q0[r]), b = std::min(q0 + nq, c->kid_q0[r + 1]);
            if (a < b) return leaf_run_resident(k, a - c->kid_q0[r], b - a, sample_proportion);
            const int rc = resolve_overflow(k);  // (an earlier call's re-runs, if it was never waited for)
            return rc ? rc : call_forgotten(k);
        });
    }
    return leaf_run_resident(c, q0, nq, sample_proportion);
}

int hvs_sync(hvs_ctx* c)
{
    if (!c) return HVS_EINVAL;
    if (!c->kids.empty()) return for_each_leaf(c, [&](uint32_t r) { return leaf_sync(c->kids[r]); });
    return leaf_sync(c);
}

int hvs_download_results(hvs_ctx* c, uint32_t q0, uint32_t nq, uint32_t* out_ids, float* out_dists)
{
    if (!c) return HVS_EINVAL;
    if (!c->kids.empty()) {
        if (!out_ids) return fail(c, HVS_EINVAL, "hvs_download_results: out_ids is NULL");
        if (c->partitioned) return part_download_results(c, q0, nq, out_ids, out_dists);
        return for_each_resident_part(c, q0, nq, [&](hvs_ctx* k, uint32_t lq0, uint32_t m, uint32_t off) {
            return leaf_download_results(k, lq0, m, out_ids + (size_t)off * c->k, out_dists ? out_dists + (size_t)off * c->k : nullptr);
        });
    }
    return leaf_download_results(c, q0, nq, out_ids, out_dists);
}

int hvs_export_results_device(hvs_ctx* c, uint32_t q0, uint32_t nq, uint32_t* d_ids, float* d_dists)
{
    if (!c) return HVS_EINVAL;
    if (!c->kids.empty()) return fail(c, HVS_EINVAL, "hvs_export_results_device: single-GPU contexts only (device pointers belong to one GPU)");
    if (!d_ids || (uint64_t)q0 + nq > user_nq(c)) return fail(c, HVS_EINVAL, "hvs_export_results_device: bad range");
    HVS_HIP(c, hipSetDevice(c->device));
    int rc = resolve_overflow(c);
    if (rc) return rc;
    if (c->qs.in.active && c->qs.in.m_cap < (size_t)c->qs.in.nuq * c->k) return fail(c, HVS_ESTATE, "hvs_export_results_device: no results (hvs_query_resident has not run)");
    HVS_HIP(c, hipMemcpyAsync(d_ids, user_ids(c) + (size_t)q0 * c->k, (size_t)nq * c->k * sizeof(uint32_t),
                              hipMemcpyDeviceToDevice, c->stream));
    if (d_dists)
        HVS_HIP(c, hipMemcpyAsync(d_dists, user_dists(c) + (size_t)q0 * c->k,
                                  (size_t)nq * c->k * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    return HVS_OK;
}

int hvs_stream_wait(hvs_ctx* c, void* stream)
{
    if (!c) return HVS_EINVAL;
    if (!c->kids.empty()) return fail(c, HVS_EINVAL, "hvs_stream_wait: single-GPU contexts only (a stream belongs to one GPU)");
    HVS_HIP(c, hipSetDevice(c->device));
    int rc = resolve_overflow(c);
    if (rc) return rc;
    return c->pipe.after_compute(c->stream, static_cast<hipStream_t>(stream));
}

int hvs_query(hvs_ctx* c, const float* q_rows, uint32_t nq, float sample_proportion, uint32_t* out_ids,
              float* out_dists)
{
    return hvs_query_after(c, q_rows, nullptr, nullptr, nullptr, nq, sample_proportion, out_ids, out_dists);
}

int hvs_query_within(hvs_ctx* c, const float* q_rows, const float* max_d2, uint32_t nq, float sample_proportion, uint32_t* out_ids,
                     float* out_dists)
{
    return hvs_query_after(c, q_rows, nullptr, nullptr, max_d2, nq, sample_proportion, out_ids, out_dists);
}

int hvs_query_after(hvs_ctx* c, const float* q_rows, const float* after_d, const uint32_t* after_i, const float* max_d2, uint32_t nq,
                    float sample_proportion, uint32_t* out_ids, float* out_dists)
{
    return hvs_query_excluding(c, q_rows, nullptr, nullptr, after_d, after_i, max_d2, nq, sample_proportion, out_ids, out_dists);
}

int hvs_query_excluding(hvs_ctx* c, const float* q_rows, const uint32_t* ex_off, const uint32_t* ex_ids, const float* after_d, const uint32_t* after_i,
                        const float* max_d2, uint32_t nq, float sample_proportion, uint32_t* out_ids, float* out_dists)
{
    if (!c) return HVS_EINVAL;
    if ((after_d == nullptr) != (after_i == nullptr)) return fail(c, HVS_EINVAL, "hvs_query_after: one of after_dists / after_ids is NULL");
    if ((ex_off == nullptr) != (ex_ids == nullptr)) return fail(c, HVS_EINVAL, "hvs_query_excluding: one of excl_offsets / excl_ids is NULL");
    // (the lists are the caller's host memory: refused here, before the resident set is replaced)
    if (ex_off && hvs_exclude_plan(ex_off, nullptr, nq, 0u, 0xFFFFFFFFu, nullptr, nullptr, nullptr) == 0xFFFFFFFFu)
        return fail(c, HVS_EINVAL, "hvs_query_excluding: excl_offsets are malformed, or a list has more than HVS_EXCLUDE_MAX entries");
    if (c->kids.empty()) return leaf_query(c, q_rows, nq, sample_proportion, out_ids, out_dists, nullptr, max_d2, after_d, after_i, ex_off, ex_ids);
    if (nq == 0) return HVS_OK;
    if (!q_rows || !out_ids) return fail(c, HVS_EINVAL, "hvs_query: q_rows / out_ids is NULL");
    const auto t0 = std::chrono::steady_clock::now();
    if (c->partitioned) {
        // all queries to every part over its own link, the resident call, each owner's merged slice home
        int rc = hvs_upload_queries(c, q_rows, nq);
        if (!rc) rc = attach_for_call(c, max_d2, after_d, after_i, nq, ex_off, ex_ids);
        if (!rc) rc = part_run(c, 0u, nq, sample_proportion);
        if (!rc) rc = part_download_results(c, 0u, nq, out_ids, out_dists);
        c->call.host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return rc;
    }
    cut_queries(c, nq);
    int rc;
    if (c->gather_mode == HVS_GATHER_DIRECT) {
        // zero-collective path: every GPU's pipeline reads its slice of the caller's queries and writes its slice of
        // the caller's result arrays
        rc = for_each_leaf(c, [&](uint32_t r) -> int {
            const uint32_t a = c->kid_q0[r], m = c->kid_q0[r + 1] - a;
            if (m == 0u) return call_forgotten(c->kids[r]);
            return leaf_query(c->kids[r], q_rows + (size_t)a * HVS_QCOLS, m, sample_proportion, out_ids + (size_t)a * c->k,
                              out_dists ? out_dists + (size_t)a * c->k : nullptr, nullptr, max_d2 ? max_d2 + a : nullptr,
                              after_d ? after_d + a : nullptr, after_i ? after_i + a : nullptr, ex_off ? ex_off + a : nullptr, ex_ids);
        });
    } else {
        // peer gather (A/B partner of the direct path): every GPU runs the same host pipeline on its slice of the caller's
        // queries, but its finished pieces travel GPU -> GPU 0 over xGMI under the next batch's compute (PeerSink) instead
        // of going to the host; the gathered block leaves GPU 0 in one D2H.  GPU 0's own slice starts at row 0 of its
        // result buffer, which holds everybody's rows.
        hvs_ctx* k0 = c->kids[0];
        (void)hipSetDevice(k0->device);
        rc = ensure_results(k0, nq);
        if (rc) rc = fail(c, rc, k0->err);
        if (!rc)
            rc = for_each_leaf(c, [&](uint32_t r) -> int {
                const uint32_t a = c->kid_q0[r], m = c->kid_q0[r + 1] - a;
                hvs_ctx* k = c->kids[r];
                if (m == 0u) return call_forgotten(k);
                if (r == 0u) {  // its results are already where the gather wants them: plain resident run of its slice
                    int r2 = leaf_upload_queries(k, q_rows, m);
                    if (r2) return r2;
                    if ((r2 = attach_for_call(k, max_d2, after_d, after_i, m, ex_off, ex_ids))) return r2;
                    if ((r2 = run_queries(k, 0, m, sample_proportion, NoHook{}))) return r2;
                    return leaf_sync(k);
                }
                const PeerSink sink{k0, a, out_dists != nullptr};
                return leaf_query(k, q_rows + (size_t)a * HVS_QCOLS, m, sample_proportion, nullptr, nullptr, &sink, max_d2 ? max_d2 + a : nullptr,
                                  after_d ? after_d + a : nullptr, after_i ? after_i + a : nullptr, ex_off ? ex_off + a : nullptr, ex_ids);
            });
        if (!rc) {
            (void)hipSetDevice(k0->device);
            if (hipMemcpyAsync(out_ids, k0->d_out_ids, (size_t)nq * c->k * sizeof(uint32_t), hipMemcpyDeviceToHost, k0->stream) != hipSuccess ||
                (out_dists && hipMemcpyAsync(out_dists, k0->d_out_dists, (size_t)nq * c->k * sizeof(float), hipMemcpyDeviceToHost,
                                             k0->stream) != hipSuccess) ||
                hipStreamSynchronize(k0->stream) != hipSuccess)
                rc = fail(c, HVS_EHIP, "hvs_query: download of the gathered results failed");
        }
    }
    c->call.host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

int hvs_merge_shards_device(hvs_ctx* c, uint32_t nshards, uint32_t nq, const uint32_t* d_ids_all, const float* d_dists_all,
                            const uint64_t* shard_row0, uint32_t n_total, const float* d_pad_dists, uint32_t* d_out_ids,
                            float* d_out_dists)
{
    if (!c) return HVS_EINVAL;
    if (!c->kids.empty()) return fail(c, HVS_EINVAL, "hvs_merge_shards_device: single-GPU contexts only");
    if (!d_ids_all || !d_dists_all || !shard_row0 || !d_pad_dists || !d_out_ids || nshards == 0u || nshards > 16u ||
        n_total < c->k)
        return fail(c, HVS_EINVAL, "hvs_merge_shards_device: bad argument (1..16 shards, n_total >= k, non-NULL buffers)");
    if (nq == 0u) return HVS_OK;
    HVS_HIP(c, hipSetDevice(c->device));
    HvsShardRows rows{};
    for (uint32_t s = 0; s < nshards; ++s) {
        if (shard_row0[s] >= n_total) return fail(c, HVS_EINVAL, "hvs_merge_shards_device: shard row offset outside the data set");
        rows.row0[s] = shard_row0[s];
    }
    with_cap(c->cap, [&](auto CAPT) {
        hipLaunchKernelGGL((hvs_k_merge_shards<decltype(CAPT)::value>), dim3((nq + 3u) / 4u), dim3(256), 0, c->stream, d_ids_all, d_dists_all,
                           nshards, nq, rows, n_total, d_pad_dists, d_out_ids, d_out_dists, c->k);
    });
    HVS_HIP(c, hipGetLastError());
    return HVS_OK;
}

int hvs_last_reruns(hvs_ctx* c, int which, uint32_t* out_idx, uint32_t cap)
{
    if (!c) return HVS_EINVAL;
    if (!c->kids.empty()) return fail(c, HVS_EINVAL, "hvs_last_reruns: single-GPU contexts only");
    if (which != 0 && which != 1) return fail(c, HVS_EINVAL, "hvs_last_reruns: which is 0 (exact) or 1 (retry)");
    int rc = leaf_sync(c);
    if (rc) return rc;
    const auto [d_list, len] = c->call.reruns()[which];  // (whether or not there is a last call to report: DESIGN 3.5a)
    const uint32_t m = std::min(len, cap);
    if (m && out_idx) HVS_HIP(c, hipMemcpy(out_idx, d_list, (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return (int)len;
}

int hvs_last_timing(hvs_ctx* c, hvs_timing* out)
{
    // whole-job view: device time = the slowest GPU's, work counters summed over the GPUs that took part
    return call_stats<hvs_timing>(
        c, out, leaf_last_timing,
        [&](hvs_timing& agg, const hvs_timing& t) {
            agg.query_ms = std::max(agg.query_ms, t.query_ms);
            agg.main_kernel_ms += t.main_kernel_ms;
            agg.main_kernel_launches += t.main_kernel_launches;
            agg.nq += t.nq;
            agg.pairs += t.pairs;
            agg.scanned_pairs += t.scanned_pairs;
            agg.rescored_pairs += t.rescored_pairs;
            agg.fallback_queries += t.fallback_queries;
            agg.retry_queries += t.retry_queries;
            agg.flags |= t.flags;
            agg.untimed_launches += t.untimed_launches;
            agg.load_ms = std::max(agg.load_ms, t.load_ms);
            agg.engine = t.engine;
            agg.n_gpus += 1;
            agg.host_ms = c->call.host_ms;
        },
        [&](hvs_timing& agg) {
            // every part answered all the queries (a part outside the sampled prefix launched nothing); exchange and merge follow the slowest
            agg.query_ms += c->pinfo.exchange_ms + c->pinfo.merge_ms;
            agg.nq = c->part_call_nq;
            if (!agg.n_gpus) agg.engine = HVS_ENGINE_EXACT_SCAN;
            agg.n_gpus = (uint32_t)c->kids.size();
            agg.host_ms = c->call.host_ms;
        });
}

// ---- per-query distance caps (include/hvs.h "distance caps") --------------------

int hvs_set_max_dist2(hvs_ctx* c, const float* max_d2, uint32_t nq)
{
    if (!c) return HVS_EINVAL;
    if (!max_d2) return attach_everywhere(c, PerQuery::Caps, nullptr, nullptr, -1, 0u);
    if (int rc = check_resident_count(c, nq, "hvs_set_max_dist2")) return rc;
    return attach_everywhere(c, PerQuery::Caps, max_d2, nullptr, -1, nq);
}

int hvs_set_max_dist2_device(hvs_ctx* c, const float* d_max_d2, uint32_t nq, void* stream)
{
    if (!c) return HVS_EINVAL;
    if (!d_max_d2) return attach_everywhere(c, PerQuery::Caps, nullptr, nullptr, -1, 0u);
    int dev = 0, rc = check_resident_count(c, nq, "hvs_set_max_dist2_device");
    if (!rc && nq) rc = check_device_buffers(c, d_max_d2, nullptr, stream, "hvs_set_max_dist2_device", &dev);  // (an empty set reads nothing)
    return rc ? rc : attach_everywhere(c, PerQuery::Caps, d_max_d2, nullptr, dev, nq);
}

int hvs_within_stats(hvs_ctx* c, hvs_within_info* out)
{
    return call_stats<hvs_within_info>(
        c, out, leaf_within_stats,
        [](hvs_within_info& sum, const hvs_within_info& m) {
            sum.capped_queries += m.capped_queries;
            sum.underfull_queries += m.underfull_queries;
            sum.within_slots += m.within_slots;
        },
        [&](hvs_within_info& sum) {
            // the parts' slots are summed, the queries are the call's, and a query is under-full when the merge found fewer than
            // k keys in all parts together
            sum.capped_queries = c->qs.call_capped ? c->part_call_nq : 0u;
            sum.underfull_queries = c->qs.call_capped ? c->pinfo.padded_queries : 0u;
        });
}

void hvs_within_plan(const uint32_t* ids, const float* dists, uint32_t k, float max_d2, const uint32_t* pad_ids, const float* pad_dists,
                     int padding, uint32_t* out_ids, float* out_dists, uint32_t* n_within)
{
    if (!ids || !dists) return;
    const float cap = hvs_norm_cap(max_d2);
    const uint32_t within = plan_row(ids, dists, k, k, [&](const PlanSlot& s) { return s.dist <= cap; }, pad_ids, pad_dists, padding, out_ids, out_dists);
    if (n_within) *n_within = within;
}

// ---- per-query result cursors (include/hvs.h "per-query result cursors") --------

int hvs_set_after(hvs_ctx* c, const float* after_dists, const uint32_t* after_ids, uint32_t nq)
{
    if (!c) return HVS_EINVAL;
    if (!after_dists && !after_ids) return attach_everywhere(c, PerQuery::Cursors, nullptr, nullptr, -1, 0u);
    HVS_NO_CURSORS_ON_VECTORS(c, "hvs_set_after");
    if (!after_dists || !after_ids) return fail(c, HVS_EINVAL, "hvs_set_after: one of after_dists / after_ids is NULL");
    if (int rc = check_resident_count(c, nq, "hvs_set_after")) return rc;
    return attach_everywhere(c, PerQuery::Cursors, after_dists, after_ids, -1, nq);
}

int hvs_set_after_device(hvs_ctx* c, const float* d_after_dists, const uint32_t* d_after_ids, uint32_t nq, void* stream)
{
    if (!c) return HVS_EINVAL;
    if (!d_after_dists && !d_after_ids) return attach_everywhere(c, PerQuery::Cursors, nullptr, nullptr, -1, 0u);
    HVS_NO_CURSORS_ON_VECTORS(c, "hvs_set_after_device");
    if (!d_after_dists || !d_after_ids) return fail(c, HVS_EINVAL, "hvs_set_after_device: one of d_after_dists / d_after_ids is NULL");
    int dev = 0, rc = check_resident_count(c, nq, "hvs_set_after_device");
    if (!rc && nq) rc = check_device_buffers(c, d_after_dists, d_after_ids, stream, "hvs_set_after_device", &dev);  // (an empty set reads nothing)
    return rc ? rc : attach_everywhere(c, PerQuery::Cursors, d_after_dists, d_after_ids, dev, nq);
}

int hvs_set_after_from_results(hvs_ctx* c)
{
    if (!c) return HVS_EINVAL;
    HVS_NO_CURSORS_ON_VECTORS(c, "hvs_set_after_from_results");
    if (c->padding) return fail(c, HVS_ESTATE, "hvs_set_after_from_results: padding is on (the last slot may be a pad row)");
    if (c->kids.empty()) {
        if (!leaf_has_all_results(c)) return fail(c, HVS_ESTATE, "hvs_set_after_from_results: no results for all resident queries");
        return leaf_after_from_results(c);
    }
    const uint32_t N = (uint32_t)c->kids.size();
    if (c->kid_q0.size() != N + 1u) return fail(c, HVS_ESTATE, "hvs_set_after_from_results: no resident queries");
    if (!c->partitioned) {
        for (hvs_ctx* k : c->kids)
            if (!leaf_has_all_results(k)) return fail(c, HVS_ESTATE, "hvs_set_after_from_results: no results for all resident queries");
        return for_each_leaf(c, [&](uint32_t r) { return leaf_after_from_results(c->kids[r]); });
    }
    // row-partitioned: the merged rows of an owner's queries live on the owner (d_m_ids / d_m_dists, global ids).  Every owner
    // takes its queries' last slots, every part fetches each owner's piece with device-to-device copies on its own stream
    // (8 bytes per query, like the list exchange) and builds its cursors as seen from its first row.
    const uint32_t nq = c->kid_q0.back(), K = c->k;
    if (!c->part_timing_valid || c->qs.res_gen != c->kids[0]->qs.set_gen || !c->qs.covers(nq, K))
        return fail(c, HVS_ESTATE, "hvs_set_after_from_results: no results for all resident queries");
    int rc = for_each_leaf(c, [&](uint32_t r) -> int {
        hvs_ctx* k = c->kids[r];
        HVS_HIP(k, hipSetDevice(k->device));
        int r2 = ensure_after(k, std::max(nq, 1u));
        if (r2) return r2;
        const uint32_t a = c->kid_q0[r], own = c->kid_q0[r + 1] - a;
        if (own) {
            hipLaunchKernelGGL(hvs_k_after_from_results, dim3(hvs_ceil_div(own, 256u)), dim3(256), 0, k->stream, k->part.d_m_ids, k->part.d_m_dists,
                               own, K, k->qs.eng.d_after_dist + a, k->qs.eng.d_after_id + a);
            HVS_HIP(k, hipGetLastError());
        }
        HVS_HIP(k, hipStreamSynchronize(k->stream));
        return HVS_OK;
    });
    if (!rc)
        rc = for_each_leaf(c, [&](uint32_t r) -> int {
            hvs_ctx* k = c->kids[r];
            HVS_HIP(k, hipSetDevice(k->device));
            for (uint32_t p = 0; p < N; ++p) {
                const uint32_t a = c->kid_q0[p], own = c->kid_q0[p + 1] - a;
                if (p == r || own == 0u) continue;
                const hvs_ctx* src = c->kids[p];
                HVS_HIP(k, hipMemcpyPeerAsync(k->qs.eng.d_after_dist + a, k->device, src->qs.eng.d_after_dist + a, src->device, (size_t)own * sizeof(float), k->stream));
                HVS_HIP(k, hipMemcpyPeerAsync(k->qs.eng.d_after_id + a, k->device, src->qs.eng.d_after_id + a, src->device, (size_t)own * sizeof(uint32_t), k->stream));
            }
            return leaf_attach(k, PerQuery::Cursors, PerQuerySource{PerQuerySource::InPlace}, nq, c->part_row0[r]);
        });
    if (rc) {
        part_quiesce(c);
        for (hvs_ctx* k : c->kids) k->qs.after_set = false;  // (some parts may hold the new cursors and some the old: none is in force)
    }
    return rc;
}

int hvs_after_stats(hvs_ctx* c, hvs_after_info* out)
{
    uint32_t part_exhausted = 0;
    return call_stats<hvs_after_info>(
        c, out, leaf_after_stats,
        [&](hvs_after_info& sum, const hvs_after_info& m) {
            sum.cursor_queries += m.cursor_queries;
            sum.exhausted_queries += m.exhausted_queries;
            sum.underfull_queries += m.underfull_queries;
            sum.after_slots += m.after_slots;
            part_exhausted = std::max(part_exhausted, m.exhausted_queries);
        },
        [&](hvs_after_info& sum) {
            // the rules of hvs_within_stats; every part saw every cursor, so one part's count of exhausted ones
            const bool on = c->qs.call_after;
            sum.cursor_queries = on ? c->part_call_nq : 0u;
            sum.underfull_queries = on ? c->pinfo.padded_queries : 0u;
            sum.exhausted_queries = on ? part_exhausted : 0u;
        });
}

void hvs_after_plan(const uint32_t* ids, const float* dists, uint32_t m, uint32_t k, float after_dist, uint32_t after_id, const uint32_t* pad_ids,
                    const float* pad_dists, int padding, uint32_t* out_ids, float* out_dists, uint32_t* n_after)
{
    if (m && (!ids || !dists)) return;
    const uint64_t lo = hvs_after_lo(after_dist, after_id, 0u);
    const uint32_t after = plan_row(ids, dists, m, k, [&](const PlanSlot& s) { return s.key >= lo; }, pad_ids, pad_dists, padding, out_ids, out_dists);
    if (n_after) *n_after = after;
}

// ---- per-query exclusion lists (include/hvs.h "per-query exclusion lists") -------

static_assert(HVS_EXCLUDE_MAX == HVS_EXCLUDE_MAX_, "the kernels' list capacity is the contract's");

// the normalisation of per-query id lists of at most `limit` raw entries each: exclusion lists and candidate lists
static uint32_t id_lists_plan(uint32_t limit, const uint32_t* offsets, const uint32_t* ids, uint32_t nq, uint32_t row0, uint32_t n_rows, uint32_t* begin,
                              uint32_t* count, uint32_t* out_ids)
{
    if (!offsets || offsets[0] != 0u) return 0xFFFFFFFFu;
    for (uint32_t q = 0; q < nq; ++q)
        if (offsets[q + 1] < offsets[q] || offsets[q + 1] - offsets[q] > limit) return 0xFFFFFFFFu;
    uint32_t kept_all = 0;
    std::vector<uint32_t> row;
    for (uint32_t q = 0; q < nq; ++q) {
        const uint32_t a = offsets[q], len = offsets[q + 1] - a;
        uint32_t kept = 0;
        if (ids) {
            row.clear();
            for (uint32_t e = 0; e < len; ++e)
                if (hvs_exclude_keeps(ids[a + e], row0, n_rows)) row.push_back(ids[a + e] - row0);
            std::sort(row.begin(), row.end());
            row.erase(std::unique(row.begin(), row.end()), row.end());
            kept = (uint32_t)row.size();
            if (out_ids) {
                std::copy(row.begin(), row.end(), out_ids + a);
                std::fill(out_ids + a + kept, out_ids + a + len, 0xFFFFFFFFu);
            }
        }
        if (begin) begin[q] = a;
        if (count) count[q] = kept;
        kept_all += kept;
    }
    return kept_all;
}

uint32_t hvs_exclude_plan(const uint32_t* offsets, const uint32_t* ids, uint32_t nq, uint32_t row0, uint32_t n_rows, uint32_t* begin, uint32_t* count,
                          uint32_t* out_ids)
{
    return id_lists_plan(HVS_EXCLUDE_MAX, offsets, ids, nq, row0, n_rows, begin, count, out_ids);
}

// A caller's per-query arrays come from host memory or, through a *_device entry point, from device memory with the stream that
// produced them.
struct CallerSource {
    const char* fn;
    bool device;
    void* stream;
};
// one body per host / _device pair: the checks in their order, then the kind's road to every GPU
static int set_exclude_ids(hvs_ctx* c, const CallerSource& from, const char* null_text, const uint32_t* off, const uint32_t* ids, uint32_t nq)
{
    if (!c) return HVS_EINVAL;
    if (!loaded_leaf(c, from.fn)) return HVS_ESTATE;
    if (!off && !ids) return lists_everywhere(c, kExcludeLists, nullptr, nullptr, -1, 0u, true, from.fn);
    if (!off || !ids) return fail(c, HVS_EINVAL, std::string(from.fn) + null_text);
    int dev = -1, rc = check_resident_count(c, nq, from.fn);
    if (!rc && from.device) rc = check_device_buffers(c, off, ids, from.stream, from.fn, &dev);
    return rc ? rc : lists_everywhere(c, kExcludeLists, off, ids, dev, nq, true, from.fn);
}
int hvs_set_exclude_ids(hvs_ctx* c, const uint32_t* excl_offsets, const uint32_t* excl_ids, uint32_t nq)
{
    return set_exclude_ids(c, {"hvs_set_exclude_ids", false, nullptr}, ": one of excl_offsets / excl_ids is NULL", excl_offsets, excl_ids, nq);
}
int hvs_set_exclude_ids_device(hvs_ctx* c, const uint32_t* d_offsets, const uint32_t* d_ids, uint32_t nq, void* stream)
{
    return set_exclude_ids(c, {"hvs_set_exclude_ids_device", true, stream}, ": one of d_offsets / d_ids is NULL", d_offsets, d_ids, nq);
}

int hvs_exclude_stats(hvs_ctx* c, hvs_exclude_info* out)
{
    return call_stats<hvs_exclude_info>(
        c, out, leaf_exclude_stats,
        [](hvs_exclude_info& sum, const hvs_exclude_info& m) {
            sum.excluding_queries += m.excluding_queries;
            sum.underfull_queries += m.underfull_queries;
            sum.kept_slots += m.kept_slots;
            sum.refused_keys += m.refused_keys;
        },
        [&](hvs_exclude_info& sum) {
            // the rules of hvs_within_stats: slots and refused keys summed over the parts, the queries the call's, under-full from the merge
            sum.excluding_queries = c->qs.excl.call ? c->part_call_nq : 0u;
            sum.underfull_queries = c->qs.excl.call ? c->pinfo.padded_queries : 0u;
        });
}

// the lists in force as the device holds them: begin, count (nq each) and, where `cap` has room, the ids; returns their number
static int download_lists_plan(hvs_ctx* c, const ListKind& K, const char* fn, const char* what, uint32_t* begin, uint32_t* count, uint32_t* ids, uint32_t cap)
{
    if (!c) return HVS_EINVAL;
    if (!c->kids.empty()) return fail(c, HVS_EINVAL, std::string(fn) + ": single-GPU contexts only");
    const HvsQuerySet& s = c->qs;
    const HvsIdLists& L = s.*K.lists;
    if (!L.set) return fail(c, HVS_ESTATE, std::string(fn) + ": no " + what + " lists are attached");
    const HvsListIndex& at = !K.cursor_forms ? s.cand_at : s.in.active ? s.in.user.ex : s.eng.ex;
    HVS_HIP(c, hipSetDevice(c->device));
    if (L.nq) {
        if (begin) HVS_HIP(c, hipMemcpyAsync(begin, at.d_begin, (size_t)L.nq * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        if (count) HVS_HIP(c, hipMemcpyAsync(count, at.d_count, (size_t)L.nq * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    }
    if (ids && cap >= L.total && L.total) HVS_HIP(c, hipMemcpyAsync(ids, L.d_ids, (size_t)L.total * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    return (int)L.total;
}
int hvs_download_exclude_plan(hvs_ctx* c, uint32_t* begin, uint32_t* count, uint32_t* ids, uint32_t cap)
{
    return download_lists_plan(c, kExcludeLists, "hvs_download_exclude_plan", "exclusion", begin, count, ids, cap);
}

// ---- per-query candidate lists (include/hvs.h "per-query candidate lists") -------

static_assert(HVS_CANDIDATES_MAX == HVS_CANDIDATES_MAX_, "the kernels' list capacity is the contract's");

uint32_t hvs_candidates_plan(const uint32_t* offsets, const uint32_t* ids, uint32_t nq, uint32_t row0, uint32_t n_rows, uint32_t* begin,
                             uint32_t* count, uint32_t* out_ids)
{
    return id_lists_plan(HVS_CANDIDATES_MAX, offsets, ids, nq, row0, n_rows, begin, count, out_ids);
}

// the expanded resident set (category sets, query vectors, clauses) is attached, on every GPU or on none
static bool expanded_set_attached(const hvs_ctx* c) { return (c->kids.empty() ? c : c->kids[0])->qs.in.active; }

static int set_candidate_ids(hvs_ctx* c, const CallerSource& from, const char* null_text, const uint32_t* off, const uint32_t* ids, uint32_t nq)
{
    if (!c) return HVS_EINVAL;
    if (!loaded_leaf(c, from.fn)) return HVS_ESTATE;
    if (!off && !ids) return lists_everywhere(c, kCandidateLists, nullptr, nullptr, -1, 0u, true, from.fn);
    if (expanded_set_attached(c))
        return fail(c, HVS_ESTATE, std::string(from.fn) + ": candidate lists do not compose (yet) with category sets, query vectors or clauses");
    if (!off) return fail(c, HVS_EINVAL, std::string(from.fn) + null_text);
    int dev = -1, rc = check_resident_count(c, nq, from.fn);
    if (!rc && from.device) rc = check_device_buffers(c, off, ids, from.stream, from.fn, &dev);
    return rc ? rc : lists_everywhere(c, kCandidateLists, off, ids, dev, nq, true, from.fn);
}
int hvs_set_candidate_ids(hvs_ctx* c, const uint32_t* cand_offsets, const uint32_t* cand_ids, uint32_t nq)
{
    return set_candidate_ids(c, {"hvs_set_candidate_ids", false, nullptr}, ": cand_offsets is NULL", cand_offsets, cand_ids, nq);
}
int hvs_set_candidate_ids_device(hvs_ctx* c, const uint32_t* d_offsets, const uint32_t* d_ids, uint32_t nq, void* stream)
{
    return set_candidate_ids(c, {"hvs_set_candidate_ids_device", true, stream}, ": d_offsets is NULL", d_offsets, d_ids, nq);
}

int hvs_query_among(hvs_ctx* c, const float* q_rows, const uint32_t* cand_offsets, const uint32_t* cand_ids, const float* max_d2, uint32_t nq,
                    float sample_proportion, uint32_t* out_ids, float* out_dists)
{
    static const char* const fn = "hvs_query_among";
    if (!c) return HVS_EINVAL;
    if (!loaded_leaf(c, fn)) return HVS_ESTATE;
    if (nq == 0u) return HVS_OK;
    if (!q_rows || !out_ids) return fail(c, HVS_EINVAL, std::string(fn) + ": q_rows / out_ids is NULL");
    // checked before the resident set is replaced: a refused call changes nothing
    if (!cand_offsets || hvs_candidates_plan(cand_offsets, nullptr, nq, 0u, 0xFFFFFFFFu, nullptr, nullptr, nullptr) == 0xFFFFFFFFu)
        return fail(c, HVS_EINVAL, std::string(fn) + ": cand_offsets are missing or malformed, or a list has more than HVS_CANDIDATES_MAX entries");
    if (!cand_ids && cand_offsets[nq] > 0u) return fail(c, HVS_EINVAL, std::string(fn) + ": cand_ids is NULL");
    int rc = hvs_upload_queries(c, q_rows, nq);
    if (!rc && max_d2) rc = hvs_set_max_dist2(c, max_d2, nq);
    if (!rc) rc = hvs_set_candidate_ids(c, cand_offsets, cand_ids, nq);
    if (!rc) rc = hvs_query_resident(c, 0u, nq, sample_proportion);
    if (!rc) rc = hvs_download_results(c, 0u, nq, out_ids, out_dists);
    return rc;
}

int hvs_candidates_stats(hvs_ctx* c, hvs_candidates_info* out)
{
    return call_stats<hvs_candidates_info>(
        c, out, leaf_candidates_stats,
        [](hvs_candidates_info& sum, const hvs_candidates_info& m) {
            sum.listed_queries += m.listed_queries;
            sum.underfull_queries += m.underfull_queries;
            sum.scanned_ids += m.scanned_ids;
            sum.passing_ids += m.passing_ids;
            sum.kept_slots += m.kept_slots;
            sum.scan_ms = std::max(sum.scan_ms, m.scan_ms);
        },
        [&](hvs_candidates_info& sum) {
            // the rules of hvs_exclude_stats: ids and slots summed over the parts, the queries the call's, under-full from the merge
            sum.listed_queries = c->qs.cand.call ? c->part_call_nq : 0u;
            sum.underfull_queries = c->qs.cand.call ? c->pinfo.padded_queries : 0u;
        });
}

int hvs_download_candidates_plan(hvs_ctx* c, uint32_t* begin, uint32_t* count, uint32_t* ids, uint32_t cap)
{
    return download_lists_plan(c, kCandidateLists, "hvs_download_candidates_plan", "candidate", begin, count, ids, cap);
}

// ---- shared row sets (include/hvs.h "shared row sets") ---------------------------

static_assert(HVS_ROW_SETS_MAX == HVS_ROW_SETS_MAX_, "the kernels' set count is the contract's");

void hvs_row_sets_compact_plan(const uint64_t* bits, const uint64_t* live_bits, uint32_t n, uint32_t n_sets, uint64_t* out_bits)
{
    const size_t W = mask_words(n);
    for (uint32_t s = 0; s < n_sets; ++s) {
        const uint64_t* in = bits + (size_t)s * W;
        uint64_t* out = out_bits + (size_t)s * W;
        std::fill(out, out + W, 0ull);
        uint32_t j = 0;
        for (size_t w = 0; w < W; ++w) {
            const uint64_t set = masked_word(in, n, w);
            for (uint64_t t = masked_word(live_bits, n, w); t; t &= t - 1ull, ++j)
                if ((set >> __builtin_ctzll(t)) & 1ull) out[j >> 6] |= 1ull << (j & 63u);
        }
    }
}

// rows of the whole data set as the caller numbers them, and the sets loaded (on every GPU alike)
static uint32_t sets_total_rows(const hvs_ctx* c) { return c->partitioned ? c->part_n : mask_leaf(c)->n; }
static uint32_t sets_loaded(const hvs_ctx* c) { return mask_leaf(c)->rs.n_sets; }

static int row_sets_everywhere(hvs_ctx* c, const uint64_t* bits, int src_dev, uint32_t n_sets, const char* fn)
{
    if (n_sets > HVS_ROW_SETS_MAX) return fail(c, HVS_EINVAL, std::string(fn) + ": more than HVS_ROW_SETS_MAX sets");
    if (n_sets == 0u && bits) return fail(c, HVS_EINVAL, std::string(fn) + ": bits given for no sets");
    if ((uint64_t)n_sets * set_words_for(sets_total_rows(c)) > 0xFFFFFFFFull) return fail(c, HVS_EINVAL, std::string(fn) + ": the sets have more than 2^32 - 1 words");
    auto part_of = [&](const hvs_ctx* k, uint32_t* row0) -> uint32_t {  // a part: the whole D's rows and its first row
        *row0 = 0u;
        if (!c->partitioned) return 0u;
        const size_t r = (size_t)(std::find(c->kids.begin(), c->kids.end(), k) - c->kids.begin());
        *row0 = c->part_row0.size() > r ? c->part_row0[r] : 0u;
        return c->part_n;
    };
    const int rc = two_phase(
        c,
        [&](hvs_ctx* k) {
            uint32_t row0 = 0;
            return leaf_row_sets_prepare(k, bits, src_dev, n_sets, part_of(k, &row0));
        },
        [&](hvs_ctx* k) {
            uint32_t row0 = 0;
            const uint32_t part_rows = part_of(k, &row0);
            return leaf_row_sets_commit(k, n_sets, part_rows, row0);
        },
        free_call_scratch);
    if (!rc && !c->kids.empty()) c->qs.drop_results();  // (a row-partitioned root keeps the range of merged rows itself)
    return rc;
}

int hvs_set_row_sets(hvs_ctx* c, const uint64_t* bits, uint32_t n_sets)
{
    static const char* const fn = "hvs_set_row_sets";
    if (!c) return HVS_EINVAL;
    if (!loaded_leaf(c, fn)) return HVS_ESTATE;
    return row_sets_everywhere(c, bits, -1, n_sets, fn);
}

int hvs_set_row_sets_device(hvs_ctx* c, const uint64_t* d_bits, uint32_t n_sets, void* stream)
{
    static const char* const fn = "hvs_set_row_sets_device";
    if (!c) return HVS_EINVAL;
    if (!loaded_leaf(c, fn)) return HVS_ESTATE;
    if (!d_bits) return row_sets_everywhere(c, nullptr, -1, n_sets, fn);
    if (n_sets > HVS_ROW_SETS_MAX) return fail(c, HVS_EINVAL, std::string(fn) + ": more than HVS_ROW_SETS_MAX sets");
    int dev = 0;
    const int rc = check_device_buffers(c, d_bits, nullptr, stream, fn, &dev);
    return rc ? rc : row_sets_everywhere(c, d_bits, dev, n_sets, fn);
}

int hvs_assign_row_sets(hvs_ctx* c, uint32_t set, const uint32_t* ids, uint32_t count, int member)
{
    static const char* const fn = "hvs_assign_row_sets";
    if (!c) return HVS_EINVAL;
    if (!loaded_leaf(c, fn)) return HVS_ESTATE;
    if (!sets_loaded(c)) return fail(c, HVS_ESTATE, std::string(fn) + ": no row sets are loaded (hvs_set_row_sets)");
    if (set >= sets_loaded(c)) return fail(c, HVS_EINVAL, std::string(fn) + ": set is not below n_sets");
    if (count == 0u) return HVS_OK;
    if (!ids) return fail(c, HVS_EINVAL, std::string(fn) + ": ids is NULL");
    return on_every_leaf(c, [&](hvs_ctx* k) { return leaf_assign_row_sets(k, set, ids, count, member); });
}

int hvs_get_row_sets(hvs_ctx* c, uint64_t* bits)
{
    static const char* const fn = "hvs_get_row_sets";
    if (!c) return HVS_EINVAL;
    if (!loaded_leaf(c, fn)) return HVS_ESTATE;
    if (!sets_loaded(c)) return fail(c, HVS_ESTATE, std::string(fn) + ": no row sets are loaded (hvs_set_row_sets)");
    if (!bits) return fail(c, HVS_EINVAL, std::string(fn) + ": bits is NULL");
    hvs_ctx* k = c->kids.empty() ? c : c->kids[0];  // (every GPU holds all the sets)
    const int rc = leaf_get_row_sets(k, bits);
    return rc && k != c ? fail(c, rc, k->err) : rc;
}

// the caller's set indices (host memory, src_dev < 0, or device memory of GPU src_dev) to every GPU, or, nullptr, off every GPU.
// A replicated context cuts them by the owner ranges, a row-partitioned one gives every part all of them.  Every GPU's share is
// checked before any GPU's indices are replaced: HVS_EINVAL leaves every GPU as it was.
static int query_sets_everywhere(hvs_ctx* c, const uint32_t* idx, int src_dev, uint32_t nq, const char* fn)
{
    if (!idx) return on_every_leaf(c, [](hvs_ctx* k) { return leaf_detach_flag(k, HvsQuerySet::kRowSetsOn); });
    const std::vector<Share> sh = shares_of(c, nq);
    static const char* const bad = ": a set index is neither below n_sets nor 0xFFFFFFFF";
    int rc = stage_and_judge(c, sh, idx_stage_of, fn, Refusal{bad, bad, bad},
                             [&](const Share& s, size_t) { return leaf_query_sets_stage(s.k, idx + s.q0, src_dev, s.m); });
    return rc ? rc : commit_or_detach(c, sh, HvsQuerySet::kRowSetsOn, [&](const Share& s, size_t) { return leaf_query_sets_commit(s.k, s.m); });
}

static int set_query_row_sets(hvs_ctx* c, const CallerSource& from, const uint32_t* idx, uint32_t nq)
{
    if (!c) return HVS_EINVAL;
    if (!loaded_leaf(c, from.fn)) return HVS_ESTATE;
    if (!idx) return query_sets_everywhere(c, nullptr, -1, 0u, from.fn);
    if (!sets_loaded(c)) return fail(c, HVS_ESTATE, std::string(from.fn) + ": no row sets are loaded (hvs_set_row_sets)");
    int dev = -1, rc = check_resident_count(c, nq, from.fn);
    if (!rc && from.device) rc = check_device_buffers(c, idx, nullptr, from.stream, from.fn, &dev);
    return rc ? rc : query_sets_everywhere(c, idx, dev, nq, from.fn);
}
int hvs_set_query_row_sets(hvs_ctx* c, const uint32_t* set_of_query, uint32_t nq)
{
    return set_query_row_sets(c, {"hvs_set_query_row_sets", false, nullptr}, set_of_query, nq);
}
int hvs_set_query_row_sets_device(hvs_ctx* c, const uint32_t* d_set_of_query, uint32_t nq, void* stream)
{
    return set_query_row_sets(c, {"hvs_set_query_row_sets_device", true, stream}, d_set_of_query, nq);
}

int hvs_query_in_row_sets(hvs_ctx* c, const float* q_rows, const uint32_t* set_of_query, uint32_t nq, float sample_proportion, uint32_t* out_ids,
                          float* out_dists)
{
    static const char* const fn = "hvs_query_in_row_sets";
    if (!c) return HVS_EINVAL;
    if (!loaded_leaf(c, fn)) return HVS_ESTATE;
    if (nq == 0u) return HVS_OK;
    if (!q_rows || !out_ids || !set_of_query) return fail(c, HVS_EINVAL, std::string(fn) + ": q_rows / set_of_query / out_ids is NULL");
    // checked before the resident set is replaced: a refused call changes nothing
    if (!sets_loaded(c)) return fail(c, HVS_ESTATE, std::string(fn) + ": no row sets are loaded (hvs_set_row_sets)");
    for (uint32_t q = 0; q < nq; ++q)
        if (set_of_query[q] != 0xFFFFFFFFu && set_of_query[q] >= sets_loaded(c))
            return fail(c, HVS_EINVAL, std::string(fn) + ": a set index is neither below n_sets nor 0xFFFFFFFF");
    int rc = hvs_upload_queries(c, q_rows, nq);
    if (!rc) rc = hvs_set_query_row_sets(c, set_of_query, nq);
    if (!rc) rc = hvs_query_resident(c, 0u, nq, sample_proportion);
    if (!rc) rc = hvs_download_results(c, 0u, nq, out_ids, out_dists);
    return rc;
}

// figures of the last call on one GPU (zero unless it ran with set indices attached); the sets' own figures are the caller's to fill
static int leaf_row_sets_stats(hvs_ctx* c, hvs_row_sets_info* out)
{
    *out = hvs_row_sets_info{};
    int rc = leaf_sync(c);
    if (rc || !c->call.valid || !c->qs.call_rset) return rc;
    unsigned long long v[4] = {0, 0, 0, 0}, sink[1] = {0};
    if ((rc = call_counters(c, HVS_CNT_SET_SLOTS, v))) return rc;
    if ((rc = call_counters(c, HVS_CNT_RERUN_SINK_SET_REFUSED, sink))) return rc;  // (the exact engine's re-runs count through the sink)
    out->kept_slots = v[0];
    out->underfull_queries = (uint32_t)v[1];
    out->refused_keys = v[2] + sink[0];
    out->restricted_queries = (uint32_t)v[3];
    return in_underfull(c, &out->underfull_queries);
}

int hvs_row_sets_stats(hvs_ctx* c, hvs_row_sets_info* out)
{
    if (!c || !out) return HVS_EINVAL;
    hvs_row_sets_info sum{};
    if (c->kids.empty()) {
        if (int rc = leaf_row_sets_stats(c, &sum)) return rc;
    } else {
        bool first = true;
        for (hvs_ctx* k : c->kids) {
            hvs_row_sets_info m{};
            if (int rc = leaf_row_sets_stats(k, &m)) return fail(c, rc, k->err);
            sum.kept_slots += m.kept_slots;
            sum.refused_keys += m.refused_keys;
            // (row-partitioned: every part answers every query; the first part that took part speaks for the queries, and a
            // query is under-full when the merge of the parts padded it, the rule of hvs_exclude_stats)
            if (!c->partitioned || (first && k->call.valid && k->qs.call_rset)) {
                sum.restricted_queries += m.restricted_queries;
                first = first && !c->partitioned;
            }
            if (!c->partitioned) sum.underfull_queries += m.underfull_queries;
        }
        if (c->partitioned) sum.underfull_queries = c->qs.call_rset && c->part_timing_valid ? c->pinfo.padded_queries : 0u;
    }
    const hvs_ctx* L = mask_leaf(c);
    sum.n_sets = L->rs.n_sets;
    sum.words_per_set = L->rs.n_sets ? (uint32_t)mask_words(sets_total_rows(c)) : 0u;
    sum.bytes = (uint64_t)L->rs.n_sets * L->rs.sets_words * sizeof(uint32_t);
    *out = sum;
    return HVS_OK;
}

// ---- category sets (include/hvs.h "category sets") -------------------------------

uint32_t hvs_in_plan(const float* q_rows, const uint32_t* set_offsets, const float* set_values, uint32_t nq, uint32_t* sub_offsets, uint32_t* parent,
                     float* value)
{
    return in_plan_core(q_rows, q_rows ? q_rows + 1 : nullptr, HVS_QCOLS, set_offsets, set_values, nq, sub_offsets, parent, value, nullptr);
}

int hvs_set_category_sets(hvs_ctx* c, const uint32_t* set_offsets, const float* set_values, uint32_t nq)
{
    const int go = client_attach_begin(c, kCategorySets, false, set_offsets, !set_offsets && !set_values, nq);
    if (go != kAttach) return go;
    // format and limits hold whatever the queries' types; the sub-query count is the largest when every query tests C
    if (hvs_in_plan(nullptr, set_offsets, set_values, nq, nullptr, nullptr, nullptr) == 0xFFFFFFFFu)
        return fail(c, HVS_EINVAL, "hvs_set_category_sets: malformed offsets, a set of more than 64 distinct categories, or too many sub-queries");
    // owner ranges stay cut by user queries: each GPU takes its slice of the CSR, and plans and commits it in one pass
    return commit_everywhere_or_detach_all(c, shares_of(c, nq), [&](const Share& s, size_t) { return in_attach(s.k, set_offsets + s.q0, set_values, s.m); });
}

int hvs_query_in(hvs_ctx* c, const float* q_rows, const uint32_t* set_offsets, const float* set_values, uint32_t nq, float sample_proportion,
                 uint32_t* out_ids, float* out_dists)
{
    return client_query(
        c, kCategorySets, !set_offsets && !set_values, q_rows, nq, sample_proportion, out_ids, out_dists,
        [&] { return set_offsets && hvs_in_plan(nullptr, set_offsets, set_values, nq, nullptr, nullptr, nullptr) != 0xFFFFFFFFu; },
        [&] { return hvs_set_category_sets(c, set_offsets, set_values, nq); });
}

int hvs_in_stats(hvs_ctx* c, hvs_in_info* out)
{
    return client_stats(c, kCategorySets, out, leaf_in_stats, [](hvs_in_info& sum, const hvs_in_info& m) {
        sum.set_queries += m.set_queries;
        sum.sub_queries += m.sub_queries;
        sum.max_set = std::max(sum.max_set, m.max_set);
        sum.underfull_queries += m.underfull_queries;
        sum.merged_keys += m.merged_keys;
        sum.expand_ms = std::max(sum.expand_ms, m.expand_ms);
        sum.merge_ms = std::max(sum.merge_ms, m.merge_ms);
    });
}

int hvs_set_category_sets_device(hvs_ctx* c, const uint32_t* d_set_offsets, const float* d_set_values, uint32_t nq, void* stream)
{
    static const char* const fn = "hvs_set_category_sets_device";
    const int go = client_attach_begin(c, kCategorySets, true, d_set_offsets, !d_set_offsets && !d_set_values, nq);
    if (go != kAttach) return go;
    int dev = 0;
    if (int rc = check_device_buffers(c, d_set_offsets, d_set_values, stream, fn, &dev)) return rc;
    // the slice boundaries: offsets[first query of every GPU] and offsets[nq] come to the host (4 bytes each)
    const std::vector<Share> sh = shares_of(c, nq);
    const size_t N = sh.size();
    std::vector<uint32_t> bound(N + 1u, 0u);
    for (size_t r = 0; r <= N; ++r)
        HVS_HIP(c, hipMemcpy(&bound[r], d_set_offsets + (r < N ? sh[r].q0 : nq), sizeof(uint32_t), hipMemcpyDeviceToHost));  // (the current device is the buffers')
    bool good = bound[0] == 0u && (bound[N] == 0u || d_set_values);
    for (size_t r = 0; r < N; ++r) good = good && bound[r] <= bound[r + 1u];
    if (!good) return fail(c, HVS_EINVAL, "hvs_set_category_sets_device: malformed offsets, or values missing");
    // every GPU plans its slice; nothing is in force yet, so a refusal leaves every GPU as it was
    std::vector<InPlan> plans(N);
    struct ReleaseCopies {  // (a GPU that does not hold the buffers copied its slice: given back however the call ends)
        const std::vector<Share>& sh;
        ~ReleaseCopies()
        {
            for (const Share& s : sh) (void)in_plan_release(s.k);
        }
    } release{sh};
    int rc = on_shares(c, sh, [&](const Share& s, size_t r) {
        const int rc2 = in_begin(s.k);
        return rc2 ? rc2 : in_plan_device(s.k, d_set_offsets + s.q0, d_set_values, dev, bound[r], bound[r + 1u], s.m, &plans[r]);
    });
    if (rc) {
        (void)hipGetLastError();
        return rc;
    }
    // the limit is the host call's: the sub-queries there would be if every query tested C, over the whole context
    uint64_t all_c = 0;
    for (const InPlan& P : plans) all_c += P.dev.sub_if_all_c;
    if (all_c >= 0xFFFFFFFFull) return fail(c, HVS_EINVAL, "hvs_set_category_sets_device: too many sub-queries");
    return commit_everywhere_or_detach_all(c, sh, [&](const Share& s, size_t r) { return in_commit(s.k, kCategorySets, plans[r]); });
}

int hvs_download_in_plan(hvs_ctx* c, uint32_t* sub_offsets, uint32_t* parent, float* value, uint32_t cap)
{
    if (!c) return HVS_EINVAL;
    if (!c->kids.empty()) return fail(c, HVS_EINVAL, "hvs_download_in_plan: single-GPU contexts only");
    const HvsInSet& S = c->qs.in;
    if (!S.active || S.client->kind != HvsInSet::Sets) return fail(c, HVS_ESTATE, "hvs_download_in_plan: no category sets are attached");
    const uint32_t nsub = c->nq;
    HVS_HIP(c, hipSetDevice(c->device));
    if (sub_offsets) HVS_HIP(c, hipMemcpyAsync(sub_offsets, S.d_sub_off, ((size_t)S.nuq + 1u) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (cap >= nsub && nsub) {
        if (parent) HVS_HIP(c, hipMemcpyAsync(parent, S.d_parent, (size_t)nsub * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        if (value) HVS_HIP(c, hipMemcpyAsync(value, S.d_value, (size_t)nsub * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    }
    HVS_HIP(c, hipStreamSynchronize(c->stream));
    return (int)nsub;
}

// ---- multi-vector queries (include/hvs.h "multi-vector queries") -----------------

uint32_t hvs_vectors_check(const uint32_t* offsets, uint32_t nq) { return vec_check_core(offsets, nq, HVS_VECTORS_MAX_EXTRA); }

uint32_t hvs_vectors_plan(const uint32_t* ids, const float* dists, uint32_t m, uint32_t k, const uint32_t* pad_ids, const float* pad_dists, int padding,
                          uint32_t* out_ids, float* out_dists, uint32_t* n_duplicates)
{
    if (m && k && (!ids || !dists)) return 0u;
    std::vector<PlanSlot> all;
    for (size_t j = 0; j < (size_t)m * k; ++j)
        if (ids[j] != 0xFFFFFFFFu) all.push_back(plan_slot(dists[j], ids[j]));
    // by (id, key): the first of every run of one id is the row's smallest key
    std::sort(all.begin(), all.end(), [](const PlanSlot& a, const PlanSlot& b) { return a.id != b.id ? a.id < b.id : a.key < b.key; });
    std::vector<PlanSlot> rows;
    for (const PlanSlot& s : all)
        if (rows.empty() || rows.back().id != s.id) rows.push_back(s);
    if (n_duplicates) *n_duplicates = (uint32_t)(all.size() - rows.size());
    std::sort(rows.begin(), rows.end(), [](const PlanSlot& a, const PlanSlot& b) { return a.key < b.key; });
    std::vector<uint32_t> rid(rows.size());
    std::vector<float> rd(rows.size());
    for (size_t j = 0; j < rows.size(); ++j) rid[j] = rows[j].id, rd[j] = rows[j].dist;
    return plan_row(rid.data(), rd.data(), (uint32_t)rows.size(), k, [](const PlanSlot&) { return true; }, pad_ids, pad_dists, padding, out_ids, out_dists);
}

int hvs_set_query_vectors(hvs_ctx* c, const uint32_t* vec_offsets, const float* vecs, uint32_t nq)
{
    const int go = client_attach_begin(c, kQueryVectors, false, vec_offsets, !vec_offsets && !vecs, nq);
    return go != kAttach ? go : expanded_everywhere(c, kQueryVectors, vec_offsets, {vecs, nullptr, -1}, nq, "hvs_set_query_vectors");
}

int hvs_set_query_vectors_device(hvs_ctx* c, const uint32_t* d_offsets, const float* d_vecs, uint32_t nq, void* stream)
{
    static const char* const fn = "hvs_set_query_vectors_device";
    const int go = client_attach_begin(c, kQueryVectors, true, d_offsets, !d_offsets && !d_vecs, nq);
    if (go != kAttach) return go;
    int dev = 0;
    if (int rc = check_device_buffers(c, d_offsets, d_vecs, stream, fn, &dev)) return rc;
    return expanded_everywhere(c, kQueryVectors, d_offsets, {d_vecs, nullptr, dev}, nq, fn);
}

int hvs_query_vectors(hvs_ctx* c, const float* q_rows, const uint32_t* vec_offsets, const float* vecs, uint32_t nq, float sample_proportion,
                      uint32_t* out_ids, float* out_dists)
{
    return client_query(
        c, kQueryVectors, !vec_offsets && !vecs, q_rows, nq, sample_proportion, out_ids, out_dists,
        [&] { return csr_good(kQueryVectors, vec_offsets, {vecs, nullptr, -1}, nq); }, [&] { return hvs_set_query_vectors(c, vec_offsets, vecs, nq); });
}

int hvs_vectors_stats(hvs_ctx* c, hvs_vectors_info* out)
{
    return client_stats(c, kQueryVectors, out, leaf_vectors_stats, [](hvs_vectors_info& sum, const hvs_vectors_info& m) {
        sum.multi_queries += m.multi_queries;
        sum.sub_queries += m.sub_queries;
        sum.max_vectors = std::max(sum.max_vectors, m.max_vectors);
        sum.underfull_queries += m.underfull_queries;
        sum.merged_keys += m.merged_keys;
        sum.duplicate_keys += m.duplicate_keys;
        sum.expand_ms = std::max(sum.expand_ms, m.expand_ms);
        sum.merge_ms = std::max(sum.merge_ms, m.merge_ms);
    });
}

// ---- query clauses (include/hvs.h "query clauses") --------------------------------

uint32_t hvs_clauses_check(const uint32_t* offsets, uint32_t nq) { return vec_check_core(offsets, nq, HVS_CLAUSES_MAX_EXTRA); }

int hvs_set_query_clauses(hvs_ctx* c, const uint32_t* clause_offsets, const float* clause_attrs, const float* clause_vecs, uint32_t nq)
{
    const int go = client_attach_begin(c, kQueryClauses, false, clause_offsets, !clause_offsets && !clause_attrs && !clause_vecs, nq);
    return go != kAttach ? go : expanded_everywhere(c, kQueryClauses, clause_offsets, {clause_vecs, clause_attrs, -1}, nq, "hvs_set_query_clauses");
}

int hvs_set_query_clauses_device(hvs_ctx* c, const uint32_t* d_offsets, const float* d_attrs, const float* d_vecs, uint32_t nq, void* stream)
{
    static const char* const fn = "hvs_set_query_clauses_device";
    const int go = client_attach_begin(c, kQueryClauses, true, d_offsets, !d_offsets && !d_attrs && !d_vecs, nq);
    if (go != kAttach) return go;
    int dev = 0, dev3 = 0;
    if (d_vecs) {  // (the third buffer first: check_device_buffers ends with the wait for the producer)
        if (int rc = device_of_buffer(c, d_vecs, fn, &dev3)) return rc;
    }
    if (int rc = check_device_buffers(c, d_offsets, d_attrs, stream, fn, &dev)) return rc;
    if (d_vecs && dev3 != dev) return fail(c, HVS_EINVAL, "hvs_set_query_clauses_device: the buffers are on different GPUs");
    return expanded_everywhere(c, kQueryClauses, d_offsets, {d_vecs, d_attrs, dev}, nq, fn);
}

int hvs_query_clauses(hvs_ctx* c, const float* q_rows, const uint32_t* clause_offsets, const float* clause_attrs, const float* clause_vecs,
                      uint32_t nq, float sample_proportion, uint32_t* out_ids, float* out_dists)
{
    return client_query(
        c, kQueryClauses, !clause_offsets && !clause_attrs && !clause_vecs, q_rows, nq, sample_proportion, out_ids, out_dists,
        [&] { return csr_good(kQueryClauses, clause_offsets, {clause_vecs, clause_attrs, -1}, nq); },
        [&] { return hvs_set_query_clauses(c, clause_offsets, clause_attrs, clause_vecs, nq); });
}

int hvs_clauses_stats(hvs_ctx* c, hvs_clauses_info* out)
{
    return client_stats(c, kQueryClauses, out, leaf_clauses_stats, [](hvs_clauses_info& sum, const hvs_clauses_info& m) {
        sum.clause_queries += m.clause_queries;
        sum.sub_queries += m.sub_queries;
        sum.max_clauses = std::max(sum.max_clauses, m.max_clauses);
        sum.underfull_queries += m.underfull_queries;
        sum.read_keys += m.read_keys;
        sum.duplicate_keys += m.duplicate_keys;
        sum.bounded_keys += m.bounded_keys;
        sum.skipped_chunks += m.skipped_chunks;
        sum.expand_ms = std::max(sum.expand_ms, m.expand_ms);
        sum.merge_ms = std::max(sum.merge_ms, m.merge_ms);
    });
}

// ---- live-row mask ---------------------------------------------------------------------------

void hvs_mask_plan(const uint64_t* live_bits, uint32_t n, uint32_t k, float sample_proportion, uint32_t* n_live, uint32_t* cut,
                   uint32_t* pad_ids)
{
    const uint32_t words = (uint32_t)mask_words(n);
    auto word = [&](uint32_t w) { return masked_word(live_bits, n, w); };
    const uint32_t nl = live_bits ? mask_popcount(live_bits, n) : n;
    if (n_live) *n_live = nl;
    if (cut) {
        const uint32_t sn_live = sample_rows(sample_proportion, nl);
        *cut = n;  // sn_live == n_live: no row is cut off
        if (sn_live < nl) {
            uint32_t seen = 0;  // the id of live row number sn_live (counting from 0)
            for (uint32_t w = 0; w < words; ++w) {
                uint64_t v = word(w);
                const uint32_t pc = (uint32_t)__builtin_popcountll(v);
                if (seen + pc <= sn_live) {
                    seen += pc;
                    continue;
                }
                for (; seen < sn_live; ++seen) v &= v - 1ull;
                *cut = w * 64u + (uint32_t)__builtin_ctzll(v);
                break;
            }
        }
    }
    if (pad_ids) {
        uint32_t have = 0;
        for (uint32_t w = words; w > 0u && have < k; --w) {
            uint64_t v = word(w - 1u);
            while (v && have < k) {
                const uint32_t b = 63u - (uint32_t)__builtin_clzll(v);
                pad_ids[have++] = (w - 1u) * 64u + b;
                v &= ~(1ull << b);
            }
        }
        for (; have < k; ++have) pad_ids[have] = 0xFFFFFFFFu;  // fewer than k live rows (no context accepts such a mask)
    }
}

static int apply_mask_everywhere(hvs_ctx* c, const std::vector<uint64_t>& words, uint32_t n_live, const uint32_t* del_ids,
                                 uint32_t del_count)
{
    if (c->kids.empty()) return leaf_apply_mask(c, words, n_live, del_ids, del_count);
    return for_each_leaf(c, [&](uint32_t r) { return leaf_apply_mask(c->kids[r], words, n_live, del_ids, del_count); });
}

int hvs_set_row_mask(hvs_ctx* c, const uint64_t* live_bits)
{
    if (!c) return HVS_EINVAL;
    HVS_NOT_PARTITIONED(c, "hvs_set_row_mask");
    const hvs_ctx* L = loaded_leaf(c, "hvs_set_row_mask");
    if (!L) return HVS_ESTATE;
    std::vector<uint64_t> words = all_live_words(L->n);
    if (live_bits)
        for (size_t i = 0; i < words.size(); ++i) words[i] &= live_bits[i];
    const uint32_t n_live = mask_popcount(words.data(), L->n);
    if (n_live < L->k) return fail(c, HVS_EINVAL, "hvs_set_row_mask: the mask leaves fewer than k live rows");
    return apply_mask_everywhere(c, words, n_live, nullptr, 0u);
}

int hvs_delete_rows(hvs_ctx* c, const uint32_t* ids, uint32_t count)
{
    if (!c) return HVS_EINVAL;
    HVS_NOT_PARTITIONED(c, "hvs_delete_rows");
    const hvs_ctx* L = loaded_leaf(c, "hvs_delete_rows");
    if (!L) return HVS_ESTATE;
    if (count && !ids) return fail(c, HVS_EINVAL, "hvs_delete_rows: ids is NULL");
    for (uint32_t i = 0; i < count; ++i)
        if (ids[i] >= L->n) return fail(c, HVS_EINVAL, "hvs_delete_rows: id outside [0, n)");
    if (!count) return HVS_OK;
    std::vector<uint64_t> words = L->rs.h_live.empty() ? all_live_words(L->n) : L->rs.h_live;
    for (uint32_t i = 0; i < count; ++i) words[ids[i] >> 6] &= ~(1ull << (ids[i] & 63u));
    const uint32_t n_live = mask_popcount(words.data(), L->n);
    if (n_live < L->k) return fail(c, HVS_EINVAL, "hvs_delete_rows: fewer than k live rows would be left");
    return apply_mask_everywhere(c, words, n_live, ids, count);
}

int hvs_get_row_mask(hvs_ctx* c, uint64_t* live_bits)
{
    if (!c || !live_bits) return HVS_EINVAL;
    HVS_NOT_PARTITIONED(c, "hvs_get_row_mask");
    const hvs_ctx* L = loaded_leaf(c, "hvs_get_row_mask");
    if (!L) return HVS_ESTATE;
    const std::vector<uint64_t> words = L->rs.h_live.empty() ? all_live_words(L->n) : L->rs.h_live;
    std::memcpy(live_bits, words.data(), words.size() * sizeof(uint64_t));
    return HVS_OK;
}

uint32_t hvs_num_live_rows(const hvs_ctx* c)
{
    if (c && c->partitioned) return c->part_n;
    return c ? mask_leaf(c)->n - mask_leaf(c)->rs.n_dead : 0u;
}

int hvs_mask_stats(hvs_ctx* c, hvs_mask_info* out)
{
    if (c) HVS_NOT_PARTITIONED(c, "hvs_mask_stats");
    return leaf0_stats(c, out, leaf_mask_stats, [](hvs_mask_info& sum, const hvs_mask_info& m) { sum.dead_survivors += m.dead_survivors; });
}

// ---- appended rows ---------------------------------------------------------------------------

void hvs_append_plan(uint32_t n_indexed, uint32_t n_total, float sample_proportion, uint32_t* sn, uint32_t* tail_lo, uint32_t* tail_hi)
{
    const uint32_t s = sample_rows(sample_proportion, n_total);
    if (sn) *sn = s;
    if (tail_lo) *tail_lo = n_indexed;
    if (tail_hi) *tail_hi = std::max(n_indexed, s);
}

int hvs_append_rows(hvs_ctx* c, const float* rows, uint32_t count, uint32_t* first_id)
{
    if (!c) return HVS_EINVAL;
    HVS_NOT_PARTITIONED(c, "hvs_append_rows");
    if (count == 0u) return HVS_OK;
    if (!rows) return fail(c, HVS_EINVAL, "hvs_append_rows: rows is NULL");
    const hvs_ctx* L = loaded_leaf(c, "hvs_append_rows");
    if (!L) return HVS_ESTATE;
    if ((uint64_t)L->n + count > 0xFFFFFFFFull) return fail(c, HVS_EINVAL, "hvs_append_rows: more than 2^32 - 1 rows");
    const uint32_t first = L->n;
    const int rc = two_phase(c, [&](hvs_ctx* k) { return leaf_append_prepare(k, count); }, [&](hvs_ctx* k) { return leaf_append_commit(k, rows, count); });
    if (rc) return rc;
    if (first_id) *first_id = first;
    return HVS_OK;
}

int hvs_reserve_rows(hvs_ctx* c, uint32_t n_capacity)
{
    if (!c) return HVS_EINVAL;
    HVS_NOT_PARTITIONED(c, "hvs_reserve_rows");
    const int rc = on_every_leaf(c, [&](hvs_ctx* k) { return leaf_reserve_rows(k, n_capacity); });
    if (rc) (void)hipGetLastError();  // (as two_phase does)
    return rc;
}

int hvs_reindex(hvs_ctx* c)
{
    if (!c) return HVS_EINVAL;
    HVS_NOT_PARTITIONED(c, "hvs_reindex");
    return on_every_leaf(c, [&](hvs_ctx* k) { return leaf_reindex(k, false); });
}

int hvs_set_tail_limit(hvs_ctx* c, uint32_t rows)
{
    if (!c) return HVS_EINVAL;
    HVS_NOT_PARTITIONED(c, "hvs_set_tail_limit");
    c->rs.tail_limit = rows;
    for (hvs_ctx* k : c->kids) k->rs.tail_limit = rows;
    return HVS_OK;
}

int hvs_append_stats(hvs_ctx* c, hvs_append_info* out)
{
    if (c) HVS_NOT_PARTITIONED(c, "hvs_append_stats");
    return leaf0_stats(c, out, leaf_append_stats, [](hvs_append_info& sum, const hvs_append_info& m) {
        sum.tail_pairs += m.tail_pairs;
        sum.tail_admitted += m.tail_admitted;
    });
}

// ---- updated rows ----------------------------------------------------------------------------

uint32_t hvs_update_plan(const uint32_t* stale, uint32_t n_stale, const uint32_t* ids, uint32_t count, uint32_t n_indexed, uint32_t n_total,
                         uint32_t* out_stale, uint8_t* out_last)
{
    for (uint32_t i = 0; i < count; ++i)
        if (ids[i] >= n_total) return 0xFFFFFFFFu;
    // occurrences ordered by (id, place in the call): the last of every run is the one that wins
    std::vector<uint64_t> occ(count);
    for (uint32_t i = 0; i < count; ++i) occ[i] = ((uint64_t)ids[i] << 32) | i;
    std::sort(occ.begin(), occ.end());
    std::vector<uint32_t> fresh;
    for (uint32_t j = 0; j < count; ++j) {
        const bool last = j + 1u == count || (uint32_t)(occ[j + 1u] >> 32) != (uint32_t)(occ[j] >> 32);
        if (out_last) out_last[(uint32_t)occ[j]] = last ? 1u : 0u;
        if (last && (uint32_t)(occ[j] >> 32) < n_indexed) fresh.push_back((uint32_t)(occ[j] >> 32));
    }
    std::vector<uint32_t> merged;
    merged.reserve((size_t)n_stale + fresh.size());
    std::set_union(stale, stale + n_stale, fresh.begin(), fresh.end(), std::back_inserter(merged));
    if (out_stale) std::copy(merged.begin(), merged.end(), out_stale);
    return (uint32_t)merged.size();
}

int hvs_update_rows(hvs_ctx* c, const uint32_t* ids, const float* rows, uint32_t count)
{
    if (!c) return HVS_EINVAL;
    HVS_NOT_PARTITIONED(c, "hvs_update_rows");
    if (count == 0u) return HVS_OK;
    if (!ids) return fail(c, HVS_EINVAL, "hvs_update_rows: ids is NULL");
    if (!rows) return fail(c, HVS_EINVAL, "hvs_update_rows: rows is NULL");
    const hvs_ctx* L = loaded_leaf(c, "hvs_update_rows");
    if (!L) return HVS_ESTATE;
    std::vector<uint32_t> stale_new(L->rs.h_stale.size() + (size_t)count);
    std::vector<uint8_t> last(count);
    const uint32_t len = hvs_update_plan(L->rs.h_stale.data(), (uint32_t)L->rs.h_stale.size(), ids, count, L->n_indexed, L->n, stale_new.data(),
                                         last.data());
    if (len == 0xFFFFFFFFu) return fail(c, HVS_EINVAL, "hvs_update_rows: id outside [0, n)");
    stale_new.resize(len);
    std::vector<uint32_t> uids, from;  // every id once, with the place of its last occurrence
    for (uint32_t i = 0; i < count; ++i)
        if (last[i]) {
            uids.push_back(ids[i]);
            from.push_back(i);
        }
    const uint32_t nu = (uint32_t)uids.size();
    return two_phase(c, [&](hvs_ctx* k) { return leaf_update_prepare(k, count, len); },
                     [&](hvs_ctx* k) { return leaf_update_commit(k, rows, count, uids.data(), from.data(), nu, stale_new); });
}

int hvs_update_stats(hvs_ctx* c, hvs_update_info* out)
{
    if (c) HVS_NOT_PARTITIONED(c, "hvs_update_stats");
    return leaf0_stats(c, out, leaf_update_stats, [](hvs_update_info& sum, const hvs_update_info& m) {
        sum.stale_pairs += m.stale_pairs;
        sum.stale_admitted += m.stale_admitted;
        sum.stale_survivors += m.stale_survivors;
    });
}

// ---- row compaction --------------------------------------------------------------------------

void hvs_compact_plan(const uint64_t* live_bits, uint32_t n, uint32_t* n_live, uint32_t* first_dead, uint32_t* new_to_old)
{
    const uint32_t words = (uint32_t)mask_words(n);
    uint32_t nl = 0, fd = n;
    for (uint32_t w = 0; w < words; ++w) {
        const uint64_t valid = masked_word(nullptr, n, w), v = masked_word(live_bits, n, w);
        if (fd == n && v != valid) fd = w * 64u + (uint32_t)__builtin_ctzll(~v);
        if (new_to_old) {
            for (uint64_t t = v; t; t &= t - 1ull) new_to_old[nl++] = w * 64u + (uint32_t)__builtin_ctzll(t);
        } else {
            nl += (uint32_t)__builtin_popcountll(v);
        }
    }
    if (n_live) *n_live = nl;
    if (first_dead) *first_dead = fd;
}

int hvs_compact(hvs_ctx* c, uint32_t* new_to_old)
{
    if (!c) return HVS_EINVAL;
    HVS_NOT_PARTITIONED(c, "hvs_compact");
    const hvs_ctx* L = loaded_leaf(c, "hvs_compact");
    if (!L) return HVS_ESTATE;
    const uint32_t n = L->n;
    uint32_t n_live = 0, first_dead = 0;
    hvs_compact_plan(L->rs.h_live.empty() ? nullptr : L->rs.h_live.data(), n, &n_live, &first_dead, new_to_old);
    if (n_live == n) return HVS_OK;  // no dead row: nothing changes
    // live rows in front of every 32-row word of the mask
    std::vector<uint32_t> rank(((size_t)n + 31u) / 32u);
    uint32_t seen = 0;
    for (size_t w = 0; w < rank.size(); ++w) {
        rank[w] = seen;
        seen += (uint32_t)__builtin_popcount(mask_half(L->rs.h_live[w >> 1], w));
    }
    const uint32_t chunk = compact_chunk();
    return two_phase(c, [&](hvs_ctx* k) { return leaf_compact_prepare(k, first_dead, chunk); },
                     [&](hvs_ctx* k) { return leaf_compact_commit(k, rank, n_live, first_dead, chunk); }, free_call_scratch);
}

int hvs_compact_stats(hvs_ctx* c, hvs_compact_info* out)
{
    if (!c || !out) return HVS_EINVAL;
    HVS_NOT_PARTITIONED(c, "hvs_compact_stats");
    *out = mask_leaf(c)->rs.cstat;
    return HVS_OK;
}

int hvs_trim_rows(hvs_ctx* c)
{
    if (!c) return HVS_EINVAL;
    HVS_NOT_PARTITIONED(c, "hvs_trim_rows");
    if (!loaded_leaf(c, "hvs_trim_rows")) return HVS_ESTATE;
    return two_phase(c, leaf_trim_prepare, leaf_trim_commit, free_call_scratch);
}

}  // extern "C"
