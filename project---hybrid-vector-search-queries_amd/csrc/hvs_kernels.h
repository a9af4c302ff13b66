// hvs_kernels.h -- gfx950 kernels of the exact engine (FP32 exact-order scan + top-100 select).
#pragma once

#include "hvs_device.h"
#include "../../include/hvs_gen.h"

// per (query, row-chunk) candidate list capacity (keys): kernels are instantiated for CAP = 256 (k <= 128) and
// CAP = 512 (k <= 256); k itself is a run-time argument

// ---------------------------------------------------------------------------------------------
// Live-row mask (hvs_set_row_mask / hvs_delete_rows): one bit per row in u32 words, bit id & 31 of word
// id >> 5 set = row id is live.  Kernels that honour it are the MASKED = true instantiations of the exact-order kernels; the
// host launches them only while at least one row is dead, so a context without dead rows runs the code it always ran.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ bool hvs_row_live(const uint32_t* __restrict__ live, uint32_t id)
{
    return ((live[id >> 5] >> (id & 31u)) & 1u) != 0u;
}

// hvs_delete_rows: clear the bits of an id list (ids < n, checked by the host; duplicates are fine)
__global__ void hvs_k_mask_delete(const uint32_t* __restrict__ ids, uint32_t count, uint32_t* __restrict__ live)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t id = ids[i];
    atomicAnd(&live[id >> 5], ~(1u << (id & 31u)));
}

// hvs_update_rows: rows src[from[j]] of a staged block over the rows D[ids[j]] (ids < n, checked by the host; every id once:
// the host names only the last occurrence of a duplicate).  One thread per float.
__global__ void hvs_k_scatter_rows(const float* __restrict__ src, const uint32_t* __restrict__ ids, const uint32_t* __restrict__ from,
                                   uint32_t count, float* __restrict__ D)
{
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (uint64_t)count * HVS_DCOLS) return;
    const uint32_t j = (uint32_t)(e / HVS_DCOLS), col = (uint32_t)(e - (uint64_t)j * HVS_DCOLS);
    D[(size_t)ids[j] * HVS_DCOLS + col] = src[(size_t)from[j] * HVS_DCOLS + col];
}

// hvs_set_queries_from_rows: the four attribute floats [type, v, l, r] of the query built from a row with
// category C and timestamp T -- v = C where the type filters by category, l = T - dt and r = T + dt where it filters by time
// (one IEEE f32 operation each), -1 where it does not.  `type` in 0..3 (host).  hvs_row_query (host) and
// hvs_k_queries_from_rows (device) both go through here.
__host__ __device__ __forceinline__ void hvs_row_query_attrs(float C, float T, int type, float dt, float& qt, float& v, float& l, float& r)
{
    qt = (float)type;
    v = (type & 1) ? C : -1.0f;
    l = (type & 2) ? T - dt : -1.0f;
    r = (type & 2) ? T + dt : -1.0f;
}

// hvs_set_queries_from_rows: query j = [type, v, l, r, x0..x99] from row ids[j] of D (ids == nullptr: row first_id + j; ids < n
// and live, checked by the host).  A gather of 408-byte rows into 416-byte rows in 8-byte pieces: of a query's 52 pieces the
// first two are the attributes (computed from the row's piece 0 = [C, T]) and piece p >= 2 is the row's piece p - 1, bit for bit.
// One wave per HVS_ROWQ_WAVE_ROWS consecutive queries, one piece per lane and query, every load issued before the first
// store; the id is the same for the whole wave (a scalar load).  Lanes 52..63 sit out.
#define HVS_ROW_U2 (HVS_DCOLS / 2u)   // 8-byte pieces per row
#define HVS_QROW_U2 (HVS_QCOLS / 2u)  // ... per query row
#define HVS_ROWQ_WAVE_ROWS 4u
__global__ __launch_bounds__(256) void hvs_k_queries_from_rows(const uint2* __restrict__ D, const uint32_t* __restrict__ ids, uint32_t first_id,
                                                              uint32_t nq, int type, float dt, uint2* __restrict__ Q)
{
    static_assert(HVS_DCOLS % 2u == 0u && HVS_QCOLS == HVS_DCOLS + 2u && HVS_QROW_U2 <= 64u, "rows are moved in 8-byte pieces, one per lane");
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t q0 = __builtin_amdgcn_readfirstlane((blockIdx.x * 4u + (threadIdx.x >> 6)) * HVS_ROWQ_WAVE_ROWS);  // (wave-uniform)
    if (q0 >= nq || lane >= HVS_QROW_U2) return;
    const uint32_t piece = lane < 2u ? 0u : lane - 1u;
    uint2 v[HVS_ROWQ_WAVE_ROWS];
#pragma unroll
    for (uint32_t i = 0; i < HVS_ROWQ_WAVE_ROWS; ++i) {
        if (q0 + i < nq) {
            const uint32_t id = ids ? ids[q0 + i] : first_id + q0 + i;
            v[i] = D[(size_t)id * HVS_ROW_U2 + piece];
        }
    }
#pragma unroll
    for (uint32_t i = 0; i < HVS_ROWQ_WAVE_ROWS; ++i) {
        if (q0 + i < nq) {
            uint2 o = v[i];
            if (lane < 2u) {
                float qt, qv, ql, qr;
                hvs_row_query_attrs(__uint_as_float(v[i].x), __uint_as_float(v[i].y), type, dt, qt, qv, ql, qr);
                o = lane == 0u ? make_uint2(__float_as_uint(qt), __float_as_uint(qv)) : make_uint2(__float_as_uint(ql), __float_as_uint(qr));
            }
            Q[(size_t)(q0 + i) * HVS_QROW_U2 + lane] = o;
        }
    }
}

// hvs_compact: the live rows among the source rows [a, b) of one chunk, packed in id order into `bounce`
// (the host then copies them device-to-device to their place in D).  Not in place on purpose: row live[j] goes to place
// j <= live[j], so a chunk's destination range may overlap its OWN source range (whenever few rows before it are dead) and a
// single kernel moving rows inside D would race with itself; it never reaches a later chunk's source rows.
// One wave per 32-row mask word: the word's rows are 32 x 51 = 1632 consecutive 8-byte pieces of D (rows are 408 B, 8-byte
// aligned), read 64 pieces per instruction in two rounds of 13 loads in flight; a lane whose piece belongs to a dead row
// (or to a row outside [a, b)) sits out.  A live row's place: `rank[w]` = live rows in front of word w (host-built), plus
// the popcount of the word's bits below the row, minus rank_a = live rows in front of a.  `live`: bits past n are clear
// and b <= n (host), so nothing outside D is read; at most b - a rows of `bounce` are written.
__global__ __launch_bounds__(256) void hvs_k_compact_gather(const uint2* __restrict__ D, const uint32_t* __restrict__ live,
                                                           const uint32_t* __restrict__ rank, uint32_t a, uint32_t b, uint32_t rank_a,
                                                           uint2* __restrict__ bounce)
{
    static_assert(HVS_DCOLS % 2u == 0u, "rows are moved in 8-byte pieces");
    constexpr uint32_t E = 32u * HVS_ROW_U2, HALF = (E + 127u) / 128u;  // pieces per word; loads per round (2 rounds x 64 lanes)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w_first = a >> 5, w_last = (b - 1u) >> 5;
    const uint32_t w = w_first + blockIdx.x * 4u + (threadIdx.x >> 6);  // (wave-uniform)
    if (w > w_last) return;
    const uint32_t bits = live[w];
    uint32_t m = bits;  // the rows of this word the chunk moves
    if (w == w_first) m &= ~0u << (a & 31u);
    if (w == w_last && (b & 31u)) m &= (1u << (b & 31u)) - 1u;
    if (m == 0u) return;
    const uint32_t base = rank[w] - rank_a;  // (may wrap for the chunk's first word: the sum below does not)
    const uint2* __restrict__ src = D + (size_t)w * E;
#pragma unroll
    for (uint32_t h = 0; h < 2u; ++h) {
        uint2 v[HALF];
        uint32_t ok = 0u;
#pragma unroll
        for (uint32_t i = 0; i < HALF; ++i) {
            const uint32_t e = (h * HALF + i) * 64u + lane;
            const uint32_t r = e < E ? e / HVS_ROW_U2 : 0u;
            if (e < E && ((m >> r) & 1u)) {
                v[i] = src[e];
                ok |= 1u << i;
            }
        }
#pragma unroll
        for (uint32_t i = 0; i < HALF; ++i) {
            const uint32_t e = (h * HALF + i) * 64u + lane;
            const uint32_t r = e < E ? e / HVS_ROW_U2 : 0u;
            if ((ok >> i) & 1u) {
                const uint32_t row = base + (uint32_t)__popc(bits & ((1u << r) - 1u));
                bounce[(size_t)row * HVS_ROW_U2 + (e - r * HVS_ROW_U2)] = v[i];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Per-query distance caps (hvs_set_max_dist2 / hvs_query_within): one f32 per resident query, a squared L2
// distance; a row takes part in the query's answer only if `dist <= cap` holds for its exact-order distance (so a row with
// a NaN distance is within no cap, +inf included).  A cap that is NaN or negative matches nothing: hvs_k_norm_caps turns both
// into HVS_CAP_NOTHING once, when the caps are attached, so that every kernel needs the one compare.  Kernels that honour
// caps are the CAPPED = true instantiations of the kernels concerned (the MASKED pattern above); the host launches them only
// while caps are set, so a context without caps runs the code it always ran.
// ---------------------------------------------------------------------------------------------
#define HVS_CAP_NOTHING (-1.0f)  // `dist <= -1` is false for every distance (distances are >= 0 or NaN)
__host__ __device__ __forceinline__ float hvs_norm_cap(float c) { return c >= 0.0f ? c : HVS_CAP_NOTHING; }  // (-0 stays: 0 <= -0)
__global__ void hvs_k_norm_caps(float* __restrict__ caps, uint32_t nq)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nq) caps[i] = hvs_norm_cap(caps[i]);
}

// ---------------------------------------------------------------------------------------------
// Per-query result cursors (hvs_set_after / hvs_query_after): one key (after_dist, after_id) per resident query;
// a row takes part in the query's answer only if its key (hvs_make_key: distance bits, then id) is strictly greater.  The
// device keeps `lo[q]` = the cursor's key + 1, so that the whole test is `key >= lo[q]`, one 64-bit compare; an exhausted
// cursor (after_id = 0xFFFFFFFF) gives lo = ~0, the empty-slot key, which no row has.  hvs_k_norm_after builds lo once, when
// the cursors are attached.  `row0`: the first global row of a part of a row-partitioned context (0 otherwise) -- the cursor
// names a GLOBAL id and the part's keys carry local ones, so a cursor row in front of the part admits every local row at the
// cursor's distance (local id 0 on) and one inside or behind it admits the local ids above after_id - row0.
// Kernels that honour cursors are the AFTER = true instantiations of the kernels concerned (the MASKED / CAPPED pattern
// above); the host launches them only while cursors are set.  Unlike a cap a cursor is tested at EVERY admission into a
// candidate list: a list that admitted keys in front of the cursor would keep exactly those and prune the wanted ones.
// ---------------------------------------------------------------------------------------------
#define HVS_AFTER_NOTHING (~0ull)
__host__ __device__ __forceinline__ uint64_t hvs_after_lo(float dist, uint32_t id, uint32_t row0)
{
    if (id == 0xFFFFFFFFu) return HVS_AFTER_NOTHING;
    const uint32_t bits = (dist != dist) ? 0x7FC00000u : __builtin_bit_cast(uint32_t, dist);
    if (id < row0) return (uint64_t)bits << 32;
    return (((uint64_t)bits << 32) | (uint64_t)(id - row0)) + 1ull;  // (id - row0 < 0xFFFFFFFF: no carry into the distance)
}
__global__ void hvs_k_norm_after(const float* __restrict__ dists, const uint32_t* __restrict__ ids, uint32_t nq, uint32_t row0,
                                 uint64_t* __restrict__ lo)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nq) lo[i] = hvs_after_lo(dists[i], ids[i], row0);
}
// hvs_set_after_from_results: the last slot of `nq` result rows of `knn` slots (padding off: the largest key held, or the
// empty slot 0xFFFFFFFF / +inf of an under-full row -- an exhausted cursor) as raw cursors, for hvs_k_norm_after
__global__ void hvs_k_after_from_results(const uint32_t* __restrict__ out_ids, const float* __restrict__ out_dists, uint32_t nq,
                                         uint32_t knn, float* __restrict__ dists, uint32_t* __restrict__ ids)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const size_t last = (size_t)i * knn + (knn - 1u);
    ids[i] = out_ids[last];
    dists[i] = out_dists[last];
}

// ---------------------------------------------------------------------------------------------
// Per-query exclusion lists (hvs_set_exclude_ids / hvs_query_excluding): a set of row ids per resident query; a
// row takes part in the query's answer only if its id is not in the set.  The caller's CSR is put on the device as it is
// (hvs_k_check_offsets looks at the offsets, the host reads the status block back and refuses before anything changes), then
// hvs_k_norm_exclude sorts every list and drops what cannot name a row, IN PLACE: the normalised list of query q lies at
// ids[begin[q] .. begin[q] + count[q]), ascending and without duplicates, begin[q] = offsets[q] - offsets[0].  hvs_exclude_norm_row
// is the arithmetic of one list on the host (hvs_exclude_plan), which the kernel reproduces bit for bit.
// Kernels that honour lists are the EXCL = true instantiations of the CURSOR forms (EXCL requires AFTER: lists without cursors
// run them with an after_lo of zeros, which admits every key).  Like a cursor a list is tested at EVERY admission into a
// candidate list -- the keys it refuses are in the middle of the key order, not at its end -- but only for a key that every
// other test has admitted (hvs_refuse_listed), so it costs nothing per scanned row.  A listed id is only ever compared with a
// row's id: nothing is indexed with it.
// ---------------------------------------------------------------------------------------------
#define HVS_EXCLUDE_MAX_ 1024u  // (= HVS_EXCLUDE_MAX of include/hvs.h; hvs.hip asserts it)
#define HVS_OFF_BAD_FIRST 1u    // status flags of hvs_k_check_offsets: offsets[0] != 0
#define HVS_OFF_BAD_ORDER 2u    // ... a descending pair of offsets
#define HVS_OFF_BAD_LONG 4u     // ... a list longer than the kind's limit
struct HvsExcl {
    const uint32_t* __restrict__ begin;  // per resident query (under category sets: per sub-query, its parent's pair)
    const uint32_t* __restrict__ count;
    const uint32_t* __restrict__ ids;
    // Shared row sets ride in the same parameter: set_of[q] is the set of resident query q (under the expanded set:
    // of sub-query q, its parent's) or 0xFFFFFFFF for "no restriction"; nullptr while no query carries one.  Set s lies at
    // set_bits[s * set_words ..), one bit per GLOBAL row (row i: bit i & 31 of word i >> 5), and the kernel's row ids start at
    // global row `row0` (a part of a row-partitioned context; 0 otherwise).  The word index is formed in 64 bits.
    const uint32_t* __restrict__ set_of;
    const uint32_t* __restrict__ set_bits;
    uint32_t set_words;
    uint32_t row0;
};
// the set's admission test: is row `id` of this GPU in query qi's set?  One 4-byte load per key that everything else admitted.
__device__ __forceinline__ bool hvs_in_row_set(const HvsExcl& x, uint32_t qi, uint32_t id)
{
    if (x.set_of == nullptr) return true;
    const uint32_t s = x.set_of[qi];
    if (s == 0xFFFFFFFFu) return true;
    const uint32_t g = x.row0 + id;
    return ((x.set_bits[(size_t)s * x.set_words + (g >> 5)] >> (g & 31u)) & 1u) != 0u;
}
// an id takes part in a list normalised for rows [row0, row0 + n_rows): not the empty slot's id, and inside the window
__host__ __device__ __forceinline__ bool hvs_exclude_keeps(uint32_t id, uint32_t row0, uint32_t n_rows)
{
    return id != 0xFFFFFFFFu && id >= row0 && (uint64_t)id < (uint64_t)row0 + n_rows;
}
// The one check of a caller's CSR offsets, whatever they delimit (exclusion and candidate lists, extra vectors, extra clauses):
// status[0] |= HVS_OFF_BAD_*, status[1] = offsets[0], status[2] = offsets[nq] (to be trusted only if no flag is set).  `first`:
// the offsets are the head of the caller's array (a slice further in starts anywhere); `limit`: the longest list allowed.
__global__ void hvs_k_check_offsets(const uint32_t* __restrict__ off, uint32_t nq, int first, uint32_t limit, uint32_t* __restrict__ status)
{
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t flags = 0u;
    if (q == 0u) {
        if (first && off[0] != 0u) flags |= HVS_OFF_BAD_FIRST;
        status[1] = off[0];
        status[2] = off[nq];
    }
    if (q < nq) {
        const uint32_t a = off[q], b = off[q + 1u];
        if (b < a)
            flags |= HVS_OFF_BAD_ORDER;
        else if (b - a > limit)
            flags |= HVS_OFF_BAD_LONG;
    }
    if (flags) atomicOr(&status[0], flags);
}
// One wave per query, four queries per block, the list in LDS (4 KB per wave): ids that name no row of the window leave as
// 0xFFFFFFFF (which sorts last), the rest minus row0 are sorted by a bitonic network over the next power of two >= 64, then
// the first of every run of equal ids is kept by a ballot compaction and written back over the raw list; what is left of the
// raw length is filled with 0xFFFFFFFF, so that the whole id array is defined.  The offsets were checked: len <= 1024.
__global__ __launch_bounds__(256) void hvs_k_norm_exclude(const uint32_t* __restrict__ off, uint32_t nq, uint32_t* __restrict__ ids,
                                                          uint32_t row0, uint32_t n_rows, uint32_t* __restrict__ begin,
                                                          uint32_t* __restrict__ count)
{
    __shared__ uint32_t sids[4][HVS_EXCLUDE_MAX_];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (q >= nq) return;  // wave-uniform; waves never meet at a barrier
    uint32_t* s = sids[threadIdx.x >> 6];
    const uint32_t base = off[q] - off[0];
    uint32_t len = off[q + 1u] - off[q];
    if (len > HVS_EXCLUDE_MAX_) len = HVS_EXCLUDE_MAX_;  // (refused by the host before this launch; never trusted here)
    uint32_t* __restrict__ mine = ids + base;
    uint32_t P = 64u;
    while (P < len) P <<= 1;
    for (uint32_t e = lane; e < P; e += 64u) {
        const uint32_t id = e < len ? mine[e] : 0xFFFFFFFFu;
        s[e] = hvs_exclude_keeps(id, row0, n_rows) ? id - row0 : 0xFFFFFFFFu;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    for (uint32_t k = 2u; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
            for (uint32_t i = lane; i < P; i += 64u) {
                const uint32_t l = i ^ j;
                if (l > i) {
                    const uint32_t a = s[i], b = s[l];
                    if ((a > b) == ((i & k) == 0u)) {
                        s[i] = b;
                        s[l] = a;
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        }
    }
    uint32_t kept = 0;
    for (uint32_t off0 = 0; off0 < len; off0 += 64u) {  // (wave-uniform; s[e] for e >= len is 0xFFFFFFFF after the sort)
        const uint32_t e = off0 + lane;
        const uint32_t id = e < len ? s[e] : 0xFFFFFFFFu;
        const bool in = id != 0xFFFFFFFFu && (e == 0u || s[e - 1u] != id);
        const uint64_t m = __ballot(in);
        if (in) mine[kept + hvs_prefix_count(m)] = id;
        kept += (uint32_t)__popcll(m);
    }
    for (uint32_t e = kept + lane; e < len; e += 64u) mine[e] = 0xFFFFFFFFu;
    if (lane == 0u) {
        begin[q] = base;
        count[q] = kept;
    }
}
// under category sets every sub-query reads its parent's list: the pair is copied, the ids are not
__global__ void hvs_k_expand_exclude(const uint32_t* __restrict__ parent, uint32_t nsub, const uint32_t* __restrict__ ubegin,
                                     const uint32_t* __restrict__ ucount, uint32_t* __restrict__ begin, uint32_t* __restrict__ count)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nsub) return;
    begin[i] = ubegin[parent[i]];
    count[i] = ucount[parent[i]];
}
// the admission test: is `id` in the ascending list ids[0 .. count)?  A branch-light lower bound over at most 1024 entries.
__device__ __forceinline__ bool hvs_excluded(const uint32_t* __restrict__ ids, uint32_t count, uint32_t id)
{
    if (count == 0u) return false;
    uint32_t lo = 0u, n = count;  // the last entry <= id, if there is one, lies in [lo, lo + n)
    while (n > 1u) {
        const uint32_t half = n >> 1;
        lo = ids[lo + half] <= id ? lo + half : lo;
        n -= half;
    }
    return ids[lo] == id;
}
// ... for a key of query `qi` that every other test has admitted.  Refused keys are counted per wave in LDS and handed over
// once at the end of the kernel (one atomic per refused key on the one global counter cost as much again as the whole call at
// 10^8 refused keys).  The LDS words belong to hvs_refused_slot, so they exist in the kernels that call it -- the list forms --
// and in no other: the plain and the cursor forms declare nothing for this and keep their code to the instruction.
// hvs_refused_begin: first thing in a list form; hvs_count_refused: where the wave has converged at its end.
__device__ __forceinline__ uint32_t* hvs_refused_slot()
{
    __shared__ uint32_t sref[16];  // one word per wave of the workgroup
    return &sref[threadIdx.x >> 6];
}
// (keys refused by a shared row set, DESIGN 3.18, are counted apart: a word per wave of their own)
__device__ __forceinline__ uint32_t* hvs_set_refused_slot()
{
    __shared__ uint32_t ssetref[16];
    return &ssetref[threadIdx.x >> 6];
}
__device__ __forceinline__ void hvs_refused_begin(uint32_t lane)
{
    if (lane == 0u) {
        *hvs_refused_slot() = 0u;
        *hvs_set_refused_slot() = 0u;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");  // (LDS operations of one wave execute in order)
}
// the list first (its refusals stay what they were), then the query's row set
__device__ __forceinline__ bool hvs_refuse_listed(const HvsExcl& x, uint32_t qi, uint32_t id)
{
    if (hvs_excluded(x.ids + x.begin[qi], x.count[qi], id)) {
        atomicAdd(hvs_refused_slot(), 1u);
        return true;
    }
    if (hvs_in_row_set(x, qi, id)) return false;
    atomicAdd(hvs_set_refused_slot(), 1u);
    return true;
}
__device__ __forceinline__ void hvs_count_refused(uint32_t lane, unsigned long long* __restrict__ counters)
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    if (lane == 0u) {
        const uint32_t n = *hvs_refused_slot();
        if (n) atomicAdd(&counters[HVS_CNT_EXCL_REFUSED], (unsigned long long)n);  // (hvs_exclude_info.refused_keys)
        const uint32_t ns = *hvs_set_refused_slot();
        if (ns) atomicAdd(&counters[HVS_CNT_SET_REFUSED], (unsigned long long)ns);  // (hvs_row_sets_info.refused_keys)
    }
}

// ---------------------------------------------------------------------------------------------
// Shared row sets (hvs_set_row_sets / hvs_set_query_row_sets): the small kernels.  The bitmaps are kept as u32
// words, `words` of them per set (the same bytes as the contract's u64 words); every kernel here checks its indices against
// the extents it is given and writes with plain vector stores or atomicOr / atomicAnd.
// ---------------------------------------------------------------------------------------------
#define HVS_ROW_SETS_MAX_ 256u  // (= HVS_ROW_SETS_MAX of include/hvs.h; hvs.hip asserts it)
// status[0] |= 1 where an index is neither < n_sets nor 0xFFFFFFFF; status[1] += queries that carry a set
__global__ void hvs_k_check_query_row_sets(const uint32_t* __restrict__ idx, uint32_t nq, uint32_t n_sets, uint32_t* __restrict__ status)
{
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const uint32_t s = idx[q];
    if (s == 0xFFFFFFFFu) return;
    if (s >= n_sets)
        atomicOr(&status[0], 1u);
    else
        atomicAdd(&status[1], 1u);
}
// under the expanded set every sub-query takes its parent's index
__global__ void hvs_k_expand_query_row_sets(const uint32_t* __restrict__ parent, uint32_t nsub, const uint32_t* __restrict__ uidx,
                                            uint32_t* __restrict__ idx)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nsub) idx[i] = uidx[parent[i]];
}
// hvs_assign_row_sets: bits of ONE set (`bits`: its first word) from an id list; ids >= rows (0xFFFFFFFF among them) are ignored
__global__ void hvs_k_row_sets_assign(const uint32_t* __restrict__ ids, uint32_t count, uint32_t rows, uint32_t* __restrict__ bits, int member)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t id = ids[i];
    if (id >= rows) return;
    if (member)
        atomicOr(&bits[id >> 5], 1u << (id & 31u));
    else
        atomicAnd(&bits[id >> 5], ~(1u << (id & 31u)));
}
// n_sets bitmaps of src_words words each to dst_words words each: the words both have are copied, with the bits at or past
// `rows` cleared; the rest of a destination set is zero.  (Load: src is the caller's array; capacity growth and trim: the old one.)
__global__ void hvs_k_row_sets_restride(const uint32_t* __restrict__ src, uint32_t src_words, uint32_t* __restrict__ dst, uint32_t dst_words,
                                        uint32_t n_sets, uint32_t rows)
{
    const uint64_t total = (uint64_t)n_sets * dst_words;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const uint32_t s = (uint32_t)(e / dst_words), w = (uint32_t)(e - (uint64_t)s * dst_words);
        uint32_t v = 0u;
        if (w < src_words && ((uint64_t)w << 5) < rows) {
            v = src[(size_t)s * src_words + w];
            if (rows - (w << 5) < 32u) v &= (1u << (rows - (w << 5))) - 1u;
        }
        dst[e] = v;
    }
}
// the bits of `bits` at the set positions of `live`, packed towards bit 0 (pext)
__host__ __device__ __forceinline__ uint32_t hvs_pack_bits(uint32_t bits, uint32_t live)
{
    uint32_t out = 0u, k = 0u;
    for (uint32_t m = live; m; m &= m - 1u, ++k) out |= ((bits >> __builtin_ctz(m)) & 1u) << k;
    return out;
}
// hvs_compact's share of ONE set: per 32-row word of the live-row mask (`live`, bits past n clear) the set's bits of the live
// rows are packed and placed at bit rank[w] (live rows in front of the word) of the zeroed bounce bitmap `out` of out_words
// words.  Two words at most take bits of one source word; atomicOr, because neighbours share them.
__global__ void hvs_k_row_sets_compact(const uint32_t* __restrict__ bits, const uint32_t* __restrict__ live, const uint32_t* __restrict__ rank,
                                       uint32_t words, uint32_t* __restrict__ out, uint32_t out_words)
{
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= words) return;
    const uint32_t lv = live[w];
    const uint32_t packed = hvs_pack_bits(bits[w], lv);
    if (packed == 0u) return;
    const uint32_t r = rank[w], o = r >> 5, sh = r & 31u;
    if (o < out_words) atomicOr(&out[o], packed << sh);
    if (sh && (packed >> (32u - sh)) && o + 1u < out_words) atomicOr(&out[o + 1u], packed >> (32u - sh));
}

// ---------------------------------------------------------------------------------------------
// Synthetic inputs generated in HBM (include/hvs_gen.h), one thread per element.
// ---------------------------------------------------------------------------------------------
// `first_row`: out[0] is element 0 of that row of the stream (a part of a row-partitioned context generates its own rows)
__global__ void hvs_k_gen_data(float* __restrict__ out, uint64_t nelem, uint64_t seed, int profile, uint32_t ncat, uint64_t first_row)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nelem; e += stride) {
        const uint64_t row = e / HVS_DCOLS;
        const uint32_t col = (uint32_t)(e - row * HVS_DCOLS);
        out[e] = hvs_gen_data_elem(seed, profile, ncat, first_row + row, col);
    }
}

__global__ void hvs_k_gen_queries(float* __restrict__ out, uint64_t nelem, uint64_t seed, int profile, uint32_t ncat,
                                  int force_type, uint64_t first_row)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nelem; e += stride) {
        const uint64_t row = e / HVS_QCOLS;
        const uint32_t col = (uint32_t)(e - row * HVS_QCOLS);
        out[e] = hvs_gen_query_elem(seed, profile, ncat, force_type, first_row + row, col);
    }
}

// ---------------------------------------------------------------------------------------------
// Query scheduling keys.  Queries are independent (optimized_parallel.hpp:91 carries no state
// between iterations), so the engine may answer them in any order: they are grouped by
// (type, v, l) so that the 64 queries of a wavefront share one predicate shape and a row that
// no lane wants is skipped by the whole wave.
// key = type:3 | float(v) as ordered u32:32 | top 29 bits of ordered(l)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t hvs_ordered_u32(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ void hvs_k_query_keys(const float* __restrict__ Q, uint32_t q0, uint32_t nq, uint64_t* __restrict__ keys,
                                 uint32_t* __restrict__ idx)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const HvsQParams p = hvs_parse_query(Q + (size_t)(q0 + i) * HVS_QCOLS);
    const uint32_t vk = (p.type == 1u || p.type == 3u) ? hvs_ordered_u32(p.vf) : 0u;
    const uint32_t lk = (p.type == 2u || p.type == 3u) ? hvs_ordered_u32(p.l) : 0u;
    keys[i] = ((uint64_t)p.type << 61) | ((uint64_t)vk << 29) | (uint64_t)(lk >> 3);
    idx[i] = q0 + i;
}

// ---------------------------------------------------------------------------------------------
// hvs_k_scan_exact_lds -- the reference's inner hot loop (optimized_parallel.hpp:100-139 +
// optimized_impl.h:54-125,284-311) re-shaped for a 64-wide wavefront:
//
//   * one LANE per QUERY: the query's 100 dims live in 100 VGPRs for the whole kernel, the
//     running threshold tau and the list fill are per-lane registers;
//   * the DATA ROWS are staged in LDS: the four waves of a workgroup (256 queries) walk the same
//     row chunk, so a block of rows is copied once per workgroup (coalesced 16-B loads,
//     double-buffered, one barrier per block) into a 16-B aligned image [x0..x99, C, T, pad, pad]
//     and every wave reads it back with broadcast ds_read_b128;
//   * predicates (C == v, l <= T <= r) are evaluated per lane on the row's C,T; a row no lane
//     accepts is skipped by the whole wave (one ballot + scalar branch);
//   * the distance is the reference's exact order (8 accumulators, no FMA);
//   * admission is the reference's strict `dist < worst` (optimized_impl.h:301): accepted pairs
//     are appended to the lane's private list in global memory; a full list is cut back to its
//     100 smallest (dist,id) keys by the whole wave (hvs_wave_select_prune), which also gives
//     the new tau.  Rows are scanned in ascending id, so a later row with dist == tau can never
//     displace a kept one under the canonical (dist asc, id asc) order.
//
// Grid: x = blocks of 4 query-waves (256 queries), y = row chunk.  Waves synchronise only at the
// staging barriers.  Output: per (chunk, query slot) a list of <= HVS_CAND_CAP keys + its fill.
// ---------------------------------------------------------------------------------------------
struct HvsPairAsScalar {  // view the lane's 50 query pairs as 100 floats
    const hvs_f2* q2;
    __device__ __forceinline__ float operator[](int i) const { return (i & 1) ? q2[i >> 1].y : q2[i >> 1].x; }
};

#ifndef HVS_LDS_ROWS
#define HVS_LDS_ROWS 16   // rows per staged block (32: 8 more staging registers, which spill at three workgroups per CU)
#endif
#define HVS_LDS_ROW_F 104  // floats per staged row (416 B, 16-B aligned)

// Exact-order distance of an LDS-staged row, software-pipelined by hand: the row's 25 ds_read_b128 rotate through three
// register sets of one b-step each (2 reads, 8 components); a set is refilled for step b + 3 as soon as step b has consumed
// it, so that six reads are in flight under every step's independent v_pk_add / v_pk_mul / v_pk_add triples.  (Left to the
// compiler the loop kept 2 reads in flight and waited for each: ~35 s_nop and 27 s_waitcnt per row.  Two double-step sets,
// 8 reads in flight, need 32 registers and two workgroups per CU: measured 0.216 against 0.237 of the FP32 peak on type-0.)
// The arithmetic and its order per accumulator are hvs_exact_dist_pk's: acc2[k] takes dims (8b + 2k, 8b + 2k + 1) for
// b = 0..11 in order, then the masked tail, then the hsum tree (optimized_impl.h:96-125, :37-47).
#define HVS_LDS_STEP(LO, HI, B)                                                                     \
    {                                                                                               \
        hvs_f2 t0 = hvs_f2{LO.x, LO.y} - q2[4 * (B) + 0], t1 = hvs_f2{LO.z, LO.w} - q2[4 * (B) + 1]; \
        hvs_f2 t2 = hvs_f2{HI.x, HI.y} - q2[4 * (B) + 2], t3 = hvs_f2{HI.z, HI.w} - q2[4 * (B) + 3]; \
        t0 = t0 * t0;                                                                               \
        t1 = t1 * t1;                                                                               \
        t2 = t2 * t2;                                                                               \
        t3 = t3 * t3;                                                                               \
        a0 = a0 + t0;                                                                               \
        a1 = a1 + t1;                                                                               \
        a2 = a2 + t2;                                                                               \
        a3 = a3 + t3;                                                                               \
    }
// one step from registers (X0, X1), then the reads that refill them (float4 index NEXT.., or none)
#define HVS_LDS_ONE(X0, X1, B, NEXT)                    \
    HVS_LDS_STEP(X0, X1, (B))                           \
    __builtin_amdgcn_sched_barrier(0);                  \
    if ((NEXT) >= 0) {                                  \
        X0 = rowp[(NEXT) >= 0 ? (NEXT) : 0];            \
        if ((NEXT) + 1 < 25) X1 = rowp[(NEXT) >= 0 ? (NEXT) + 1 : 0]; \
    }                                                   \
    __builtin_amdgcn_sched_barrier(0);
__device__ __forceinline__ float hvs_exact_dist_pk_lds(const float4* rowp, const hvs_f2* q2)
{
    hvs_f2 a0 = hvs_f2{0.0f, 0.0f}, a1 = a0, a2 = a0, a3 = a0;
    float4 A0 = rowp[0], A1 = rowp[1], B0 = rowp[2], B1 = rowp[3], C0 = rowp[4], C1 = rowp[5];
    __builtin_amdgcn_sched_barrier(0);
    HVS_LDS_ONE(A0, A1, 0, 6)
    HVS_LDS_ONE(B0, B1, 1, 8)
    HVS_LDS_ONE(C0, C1, 2, 10)
    HVS_LDS_ONE(A0, A1, 3, 12)
    HVS_LDS_ONE(B0, B1, 4, 14)
    HVS_LDS_ONE(C0, C1, 5, 16)
    HVS_LDS_ONE(A0, A1, 6, 18)
    HVS_LDS_ONE(B0, B1, 7, 20)
    HVS_LDS_ONE(C0, C1, 8, 22)
    HVS_LDS_ONE(A0, A1, 9, 24)     // A0 <- dims 96..99 (the masked tail); A1 unused
    HVS_LDS_ONE(B0, B1, 10, -1)
    HVS_LDS_ONE(C0, C1, 11, -1)
    const float4 TL = A0;
    {
        hvs_f2 t2 = hvs_f2{TL.x, TL.y} - q2[48];
        hvs_f2 t3 = hvs_f2{TL.z, TL.w} - q2[49];
        t2 = t2 * t2;
        t3 = t3 * t3;
        a2 = a2 + t2;
        a3 = a3 + t3;
    }
    const hvs_f2 s01 = a0 + a2;  // (a0+a4, a1+a5)
    const hvs_f2 s23 = a1 + a3;  // (a2+a6, a3+a7)
    const float a = s01.x + s01.y;
    const float b2 = s23.x + s23.y;
    return a + b2;
}
#undef HVS_LDS_ONE
#undef HVS_LDS_STEP

struct HvsLdsRow1 {
    const float* p;
    __device__ __forceinline__ float operator[](int i) const { return p[i]; }
};

// (three workgroups per CU = three waves per SIMD, 168 registers: the 100 query components, three register sets of row data
// in flight (hvs_exact_dist_pk_lds) and the staging registers of a 16-row block fit without spilling)
#ifndef HVS_LDS_SCAN_WGS
#define HVS_LDS_SCAN_WGS 3
#endif
// SCALAR_ORDER = false: the hot path's SIMD summation order (optimized_impl.h:96-125);
// SCALAR_ORDER = true : the baseline engine's sequential order (baseline.hpp:53-64), BASELINE.json configs[0].
// MASKED: rows whose bit in `live` is clear are skipped (the row is wave-uniform: one scalar load and branch per row);
// `sn` is then the cut id of the sampled live prefix (hvs_mask_plan)
// CAPPED: admission gains `dist <= caps[query]` beside the threshold test (`caps` is not read otherwise)
// AFTER: ... and `key >= after_lo[query]` (result cursors; `after_lo` is not read otherwise)
// EXCL (a cursor form only): ... and the row's id is not in the query's exclusion list (`excl` is not read otherwise)
template <bool SCALAR_ORDER, int CAP, bool MASKED, bool CAPPED = false, bool AFTER = false, bool EXCL = false>
__global__ __launch_bounds__(256, HVS_LDS_SCAN_WGS) void hvs_k_scan_exact_lds(
    const float* __restrict__ D, const float* __restrict__ Q, const uint32_t* __restrict__ qorder, uint32_t nq,
    uint32_t nq_pad, uint32_t sn, uint32_t rows_per_chunk, uint64_t* __restrict__ cand, uint32_t* __restrict__ cand_cnt,
    unsigned long long* __restrict__ counters, uint32_t knn, const uint32_t* __restrict__ live, const float* __restrict__ caps,
    const uint64_t* __restrict__ after_lo, HvsExcl excl)
{
    static_assert(!EXCL || AFTER, "the list forms exist on the cursor forms only");
    __shared__ float4 srow[2][HVS_LDS_ROWS * HVS_LDS_ROW_F / 4];
    const uint32_t lane = threadIdx.x & 63u;
    if constexpr (EXCL) hvs_refused_begin(lane);
    const uint32_t qwave = blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t slot = qwave * 64u + lane;
    const uint32_t chunk = blockIdx.y;
    const bool wave_active = qwave * 64u < nq;  // inactive waves still help staging and meet the barriers

    const bool have_q = slot < nq;
    const uint32_t qi = qorder[have_q ? slot : (nq - 1u)];
    const float* __restrict__ qrow = Q + (size_t)qi * HVS_QCOLS;
    HvsQParams p = hvs_parse_query(qrow);
    if (!have_q) p.type = 4u;
    hvs_f2 q2[HVS_NDIM / 2];
#pragma unroll
    for (int i = 0; i < HVS_NDIM / 4; ++i) {
        const float4 v4 = *reinterpret_cast<const float4*>(qrow + 4 + 4 * i);
        q2[2 * i] = hvs_f2{v4.x, v4.y};
        q2[2 * i + 1] = hvs_f2{v4.z, v4.w};
    }

    const uint32_t r0 = chunk * rows_per_chunk;
    uint32_t r1 = r0 + rows_per_chunk;
    if (r1 > sn || r1 < r0) r1 = sn;
    if (r0 >= r1) return;  // uniform over the workgroup

    // staging: item e = (row r, piece c): c < 25 -> floats 2+4c..5+4c of the row, c == 25 -> (C, T, 0, 0)
    constexpr uint32_t kItems = HVS_LDS_ROWS * 26u;
    float4 stg[(kItems + 255u) / 256u];
    auto load_block = [&](uint32_t j0) {
#pragma unroll
        for (uint32_t k = 0; k < (kItems + 255u) / 256u; ++k) {
            const uint32_t e = threadIdx.x + 256u * k;
            const uint32_t r = e / 26u, c = e % 26u;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (e < kItems && j0 + r < r1) {
                const float* __restrict__ src = D + (size_t)(j0 + r) * HVS_DCOLS;
                if (c < 25u) {
                    const float2 a = *reinterpret_cast<const float2*>(src + 2 + 4 * c);
                    const float2 b = *reinterpret_cast<const float2*>(src + 4 + 4 * c);
                    v = make_float4(a.x, a.y, b.x, b.y);
                } else {
                    const float2 a = *reinterpret_cast<const float2*>(src);
                    v = make_float4(a.x, a.y, 0.f, 0.f);
                }
            }
            stg[k] = v;
        }
    };
    auto store_block = [&](uint32_t buf) {
#pragma unroll
        for (uint32_t k = 0; k < (kItems + 255u) / 256u; ++k) {
            const uint32_t e = threadIdx.x + 256u * k;
            if (e < kItems) srow[buf][(e / 26u) * (HVS_LDS_ROW_F / 4) + (e % 26u)] = stg[k];
        }
    };

    uint64_t* __restrict__ mylist = cand + ((size_t)chunk * nq_pad + slot) * CAP;
    // tau = NaN until the list has been cut back once: `!(dist >= tau)` then admits EVERY passing row, +inf and NaN
    // distances included, as the reference does while its list is not full (optimized_impl.h:301-304)
    float tau = __builtin_nanf("");
    float cap = 0.0f;
    if constexpr (CAPPED) cap = caps[qi];
    uint64_t lo = 0ull;
    if constexpr (AFTER) lo = after_lo[qi];
    uint32_t cnt = 0;
    uint32_t npass = 0, nscan = 0;
    // queries are sorted by type: a wave of type-0 queries only (the exact engine's slowest class) skips the per-row predicate --
    // one LDS read with its wait at the head of every row, three compares and eight scalar mask operations
    const bool wave_all0 = __ballot(have_q && p.type != 0u) == 0ull;
    const uint32_t nhave = (uint32_t)__popcll(__ballot(have_q));

    load_block(r0);
    store_block(0u);
    __syncthreads();
    uint32_t buf = 0;
    for (uint32_t j0 = r0; j0 < r1; j0 += HVS_LDS_ROWS) {
        const bool more = j0 + HVS_LDS_ROWS < r1;
        if (more) load_block(j0 + HVS_LDS_ROWS);
        if (wave_active) {
            const uint32_t nrow = (r1 - j0) < HVS_LDS_ROWS ? (r1 - j0) : HVS_LDS_ROWS;
            for (uint32_t r = 0; r < nrow; ++r) {
                if constexpr (MASKED) {
                    if (!hvs_row_live(live, j0 + r)) continue;  // (wave-uniform)
                }
                const float4* rowp = &srow[buf][r * (HVS_LDS_ROW_F / 4)];
                bool pass;
                if (wave_all0) {  // (wave-uniform) a wave of pure k-NN queries takes every row: no attribute read, no predicate
                    pass = have_q;
                    npass += nhave;
                } else {
                    const float4 attr = rowp[25];
                    pass = hvs_row_passes(p, attr.x, attr.y);
                    const uint64_t pmask = __ballot(pass);
                    if (pmask == 0ull) continue;
                    npass += (uint32_t)__popcll(pmask);
                }
                nscan += 64u;
                float dist;
                if (SCALAR_ORDER) {
                    HvsLdsRow1 d1{reinterpret_cast<const float*>(rowp)};
                    HvsPairAsScalar q1{q2};
                    dist = hvs_scalar_order_dist(d1, q1);
                } else {
                    // packed f32 math: measured 14.0 k type-0 queries/s at D=1e7 against 12.5 k with the 300 unpacked ops
                    dist = hvs_exact_dist_pk_lds(rowp, q2);
                }
                bool admit = pass && !(dist >= tau);
                if constexpr (CAPPED) admit = admit && dist <= cap;
                if constexpr (AFTER) admit = admit && hvs_make_key(dist, j0 + r) >= lo;
                if constexpr (EXCL) {
                    if (admit && hvs_refuse_listed(excl, qi, j0 + r)) admit = false;
                }
                if (admit) {
                    mylist[cnt] = hvs_make_key(dist, j0 + r);
                    ++cnt;
                }
                uint64_t full = __ballot(cnt == (uint32_t)CAP);
                if (full != 0ull) {
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                    while (full != 0ull) {
                        const uint32_t l = (uint32_t)__builtin_ctzll(full);
                        full &= full - 1ull;
                        uint64_t* lst = cand + ((size_t)chunk * nq_pad + (qwave * 64u + l)) * CAP;
                        const uint64_t kth = hvs_wave_select_prune<CAP / 64>(lst, (uint32_t)CAP, knn, lane);
                        if (lane == l) {
                            cnt = knn;
                            tau = hvs_key_dist(kth);
                        }
                    }
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                }
            }
        }
        if (more) store_block(buf ^ 1u);
        __syncthreads();
        buf ^= 1u;
    }
    if (have_q) cand_cnt[(size_t)chunk * nq_pad + slot] = cnt;
    if constexpr (EXCL) {
        if (wave_active) hvs_count_refused(lane, counters);  // (wave-uniform)
    }
    if (wave_active && lane == 0u) {
        atomicAdd(&counters[HVS_CNT_PAIRS], (unsigned long long)npass);
        atomicAdd(&counters[HVS_CNT_SCANNED], (unsigned long long)nscan);
    }
}

// ---------------------------------------------------------------------------------------------
// hvs_k_select -- per query: merge the per-chunk candidate lists (the counterpart of
// Knn::merge, optimized_impl.h:337-385 + optimized_parallel.hpp:142-146), pad with the last
// rows of D when fewer than knn rows matched (hvs_wave_pad) and emit ids in ascending
// (dist, id) order (hvs_wave_rank_write; get_knn_sorted, optimized_impl.h:392-415).
// One wave per query, 4 queries per 256-thread block, a CAP-key LDS buffer per wave.
// ---------------------------------------------------------------------------------------------
// The final kernels' share of the caps (hvs_k_select, hvs_k_merge with CAPPED): of the wave's keys buf[0 .. cnt) -- the k
// smallest the query's rows gave -- those with `dist <= cap` are kept, packed in place in their order; returns their number.
// The keys within the cap are a prefix of the query's keys in key order, so what is left is the capped answer's matched part
// and the slots behind it are padded like any under-full answer's.  Whatever the stages in front admitted, no key beyond the
// cap passes here (nor a NaN distance: `NaN <= cap` is false).
// HVS_CNT_WITHIN_SLOTS += slots kept, HVS_CNT_WITHIN_UNDERFULL += 1 for an under-full query (hvs_within_info).
__device__ __forceinline__ uint32_t hvs_keep_within(uint64_t* buf, uint32_t cnt, float cap, uint32_t knn, uint32_t lane,
                                                    unsigned long long* __restrict__ counters, bool count)
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    uint32_t kept = 0;
    for (uint32_t off = 0; off < cnt; off += 64u) {  // (wave-uniform; a chunk's keys land at or below their own places)
        const uint32_t e = off + lane;
        const uint64_t key = e < cnt ? buf[e] : 0ull;
        const bool in = e < cnt && hvs_key_dist(key) <= cap;
        const uint64_t m = __ballot(in);
        if (in) buf[kept + hvs_prefix_count(m)] = key;
        kept += (uint32_t)__popcll(m);
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    if (count && lane == 0u) {
        if (kept) atomicAdd(&counters[HVS_CNT_WITHIN_SLOTS], (unsigned long long)kept);
        if (kept < knn) atomicAdd(&counters[HVS_CNT_WITHIN_UNDERFULL], 1ull);
    }
    return kept;
}

// The final kernels' share of the cursors (hvs_k_select, hvs_k_merge with AFTER): every stage in front admits keys >= lo only,
// so this drops nothing -- it tests defensively, as hvs_keep_within does, and counts for hvs_after_info:
// HVS_CNT_AFTER_SLOTS += slots kept, HVS_CNT_AFTER_UNDERFULL += 1 for an under-full query, HVS_CNT_AFTER_EXHAUSTED += 1 for an exhausted cursor.
__device__ __forceinline__ uint32_t hvs_keep_after(uint64_t* buf, uint32_t cnt, uint64_t lo, uint32_t knn, uint32_t lane,
                                                   unsigned long long* __restrict__ counters, bool count)
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    uint32_t kept = 0;
    for (uint32_t off = 0; off < cnt; off += 64u) {  // (wave-uniform; a chunk's keys land at or below their own places)
        const uint32_t e = off + lane;
        const uint64_t key = e < cnt ? buf[e] : 0ull;
        const bool in = e < cnt && key >= lo;
        const uint64_t m = __ballot(in);
        if (in) buf[kept + hvs_prefix_count(m)] = key;
        kept += (uint32_t)__popcll(m);
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    if (count && lane == 0u) {
        if (kept) atomicAdd(&counters[HVS_CNT_AFTER_SLOTS], (unsigned long long)kept);
        if (kept < knn) atomicAdd(&counters[HVS_CNT_AFTER_UNDERFULL], 1ull);
        if (lo == HVS_AFTER_NOTHING) atomicAdd(&counters[HVS_CNT_AFTER_EXHAUSTED], 1ull);
    }
    return kept;
}

// The final kernels' share of the exclusion lists (hvs_k_select, hvs_k_merge with EXCL): as for the cursors every stage in front
// admits unlisted keys only, so this drops nothing -- it tests defensively and counts for hvs_exclude_info:
// HVS_CNT_EXCL_SLOTS += slots kept, HVS_CNT_EXCL_UNDERFULL += 1 for an under-full query.
__device__ __forceinline__ uint32_t hvs_keep_unlisted(uint64_t* buf, uint32_t cnt, const HvsExcl& x, uint32_t qi, uint32_t knn, uint32_t lane,
                                                      unsigned long long* __restrict__ counters, bool count)
{
    const uint32_t* __restrict__ lst = x.ids + x.begin[qi];
    const uint32_t n = x.count[qi];
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    uint32_t kept = 0;
    for (uint32_t off = 0; off < cnt; off += 64u) {  // (wave-uniform; a chunk's keys land at or below their own places)
        const uint32_t e = off + lane;
        const uint64_t key = e < cnt ? buf[e] : 0ull;
        const bool in = e < cnt && !hvs_excluded(lst, n, hvs_key_id(key)) && hvs_in_row_set(x, qi, hvs_key_id(key));
        const uint64_t m = __ballot(in);
        if (in) buf[kept + hvs_prefix_count(m)] = key;
        kept += (uint32_t)__popcll(m);
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    if (count && lane == 0u) {
        if (kept) atomicAdd(&counters[HVS_CNT_EXCL_SLOTS], (unsigned long long)kept);
        if (kept < knn) atomicAdd(&counters[HVS_CNT_EXCL_UNDERFULL], 1ull);
        if (x.set_of != nullptr) {  // (shared row sets, DESIGN 3.18: the same two figures for hvs_row_sets_info)
            if (kept) atomicAdd(&counters[HVS_CNT_SET_SLOTS], (unsigned long long)kept);
            if (kept < knn) atomicAdd(&counters[HVS_CNT_SET_UNDERFULL], 1ull);
            if (x.set_of[qi] != 0xFFFFFFFFu) atomicAdd(&counters[HVS_CNT_SET_RESTRICTED], 1ull);
        }
    }
    return kept;
}

// MASKED: the padding ids come from `pad_ids` (the last k live rows, descending) instead of n - 1, n - 2, ...
// CAPPED: keys beyond caps[query] leave before the padding (hvs_keep_within; `caps` and `counters` are not read otherwise)
// AFTER: keys in front of after_lo[query] likewise (hvs_keep_after; `after_lo` is not read otherwise)
// EXCL (a cursor form only): keys of listed rows likewise (hvs_keep_unlisted; `excl` is not read otherwise)
template <bool SCALAR_ORDER, int CAP, bool MASKED, bool CAPPED = false, bool AFTER = false, bool EXCL = false>
__global__ __launch_bounds__(256) void hvs_k_select(
    const float* __restrict__ D, uint32_t n, const float* __restrict__ Q, const uint32_t* __restrict__ qorder,
    uint32_t nq, uint32_t nq_pad, uint32_t nchunks, const uint64_t* __restrict__ cand,
    const uint32_t* __restrict__ cand_cnt, int pad, uint32_t* __restrict__ out_ids, float* __restrict__ out_dists, uint32_t knn,
    const uint32_t* __restrict__ pad_ids, const float* __restrict__ caps, unsigned long long* __restrict__ counters,
    const uint64_t* __restrict__ after_lo, HvsExcl excl)
{
    static_assert(!EXCL || AFTER, "the list forms exist on the cursor forms only");
    __shared__ uint64_t sbuf[4][CAP];
    __shared__ uint32_t shist[4][256];  // digit histograms of the radix select
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = threadIdx.x >> 6;
    const uint32_t slot = blockIdx.x * 4u + w;
    if (slot >= nq) return;  // wave-uniform
    uint64_t* buf = sbuf[w];
    const uint32_t qi = qorder[slot];
    if (qi == 0xFFFFFFFFu) return;  // padding slot of the range-scan layout

    uint32_t cnt = 0;
    for (uint32_t c = 0; c < nchunks; ++c) {
        const uint32_t m = cand_cnt[(size_t)c * nq_pad + slot];
        const uint64_t* __restrict__ lst = cand + ((size_t)c * nq_pad + slot) * CAP;
        for (uint32_t off = 0; off < m; off += 64u) {
            cnt = hvs_wave_make_room<CAP>(buf, shist[w], cnt, 64u, knn, lane);
            const uint32_t take = (m - off) < 64u ? (m - off) : 64u;
            if (lane < take) buf[cnt + lane] = lst[off + lane];
            cnt += take;
        }
    }
    // hvs_wave_final_cut, written out: with the call here the compiler lays this kernel's blocks out in another order, and 34 of
    // its 48 instantiations change their register counts (profiles/merge_tail_kernel_diff.txt)
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    if (cnt > knn) {
        hvs_wave_select_prune<CAP / 64>(buf, cnt, knn, lane, shist[w]);
        cnt = knn;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    }
    if constexpr (CAPPED) cnt = hvs_keep_within(buf, cnt, caps[qi], knn, lane, counters, true);
    if constexpr (AFTER) cnt = hvs_keep_after(buf, cnt, after_lo[qi], knn, lane, counters, true);
    if constexpr (EXCL) cnt = hvs_keep_unlisted(buf, cnt, excl, qi, knn, lane, counters, true);
    // fewer than knn matching rows in [0,sn): row n - 1 - s, or the s-th of the last live rows
    const float* __restrict__ qv = Q + (size_t)qi * HVS_QCOLS + 4;
    hvs_wave_pad(buf, cnt, knn, pad, lane, [=](uint32_t s) { return hvs_row_key<SCALAR_ORDER>(D, MASKED ? pad_ids[s] : n - 1u - s, qv); });
    hvs_wave_rank_write(buf, knn, lane, qi, out_ids, out_dists);
}

// ---------------------------------------------------------------------------------------------
// hvs_k_merge_shards -- D-sharded mode: the multi-GPU counterpart of Knn::merge
// (optimized_impl.h:337-385).  Every shard (GPU) answered ALL queries on its own rows with padding off:
// ids are shard-local (0xFFFFFFFF = empty slot), lists sorted by (dist, id).  Per query (one wave): the
// nshards x knn keys (dist bits << 32 | global id) are reduced to the knn smallest; when fewer than knn rows
// matched anywhere, rows n_total-1, n_total-2, ... are appended with their exact-order distances
// (hvs_wave_pad; `pad_dists[q][s]` = distance of query q to row n_total-1-s), and the knn
// keys leave in ascending (dist, id) order.  ids_all / dists_all: [nshards][nq][knn] as all_gather lays them out.
// ---------------------------------------------------------------------------------------------
struct HvsShardRows {
    uint64_t row0[16];  // first global row of each shard
};

// One part's result row of one query -- `knn` slots, ids local to the part (0xFFFFFFFF = empty slot) -- appended to the wave's
// key buffer as (dist bits << 32 | row0 + id); `cnt` keys are held, the new count is returned.  The buffer is cut back to its
// knn smallest keys whenever the next 64 slots might not fit (hvs_wave_make_room).  Shared by the two merges over row parts
// below and by hvs_k_merge_in.
template <int CAP>
__device__ __forceinline__ uint32_t hvs_gather_list_keys(uint64_t* buf, uint32_t* hist, uint32_t cnt, const uint32_t* __restrict__ ids,
                                                         const float* __restrict__ dists, uint64_t row0, uint32_t knn, uint32_t lane)
{
    for (uint32_t off = 0; off < knn; off += 64u) {
        cnt = hvs_wave_make_room<CAP>(buf, hist, cnt, 64u, knn, lane);
        const uint32_t e = off + lane;
        const uint32_t id = e < knn ? ids[e] : 0xFFFFFFFFu;
        const bool have = id != 0xFFFFFFFFu;
        const uint64_t m = __ballot(have);
        if (have) buf[cnt + hvs_prefix_count(m)] = hvs_make_key(dists[e], (uint32_t)(row0 + id));
        cnt += (uint32_t)__popcll(m);
    }
    return cnt;
}

template <int CAP>
__global__ __launch_bounds__(256) void hvs_k_merge_shards(const uint32_t* __restrict__ ids_all,
                                                          const float* __restrict__ dists_all, uint32_t nshards,
                                                          uint32_t nq, HvsShardRows rows, uint32_t n_total,
                                                          const float* __restrict__ pad_dists,
                                                          uint32_t* __restrict__ out_ids, float* __restrict__ out_dists, uint32_t knn)
{
    __shared__ uint64_t sbuf[4][CAP];
    __shared__ uint32_t shist[4][256];  // digit histograms of the radix select
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = threadIdx.x >> 6;
    const uint32_t q = blockIdx.x * 4u + w;
    if (q >= nq) return;  // wave-uniform
    uint64_t* buf = sbuf[w];
    uint32_t cnt = 0;
    for (uint32_t s = 0; s < nshards; ++s) {
        const size_t base = ((size_t)s * nq + q) * knn;
        cnt = hvs_gather_list_keys<CAP>(buf, shist[w], cnt, ids_all + base, dists_all + base, rows.row0[s], knn, lane);
    }
    cnt = hvs_wave_final_cut<CAP>(buf, shist[w], cnt, knn, lane);
    // padding is always on here and every pad slot takes a row's key, so the key ~0 that hvs_wave_rank_write turns into +inf
    // never reaches it: the distances leave as their bits
    hvs_wave_pad(buf, cnt, knn, 1, lane, [=](uint32_t s) { return hvs_make_key(pad_dists[(size_t)q * knn + s], n_total - 1u - s); });
    hvs_wave_rank_write(buf, knn, lane, q, out_ids, out_dists);
}

// ---------------------------------------------------------------------------------------------
// hvs_k_merge_parts -- row-partitioned context (include/hvs.h "row-partitioned context"): the owner of a query range
// merges the parts' partial answers for its queries and applies the reference's padding once.  Every part answered the
// queries on its own rows with padding off: ids part-local, 0xFFFFFFFF = empty slot.  `parts` names, per part, its result rows
// of the owner's queries (row i = query i of the range: the owner's own result buffer, or the gather buffer the other parts'
// rows were copied into) and its first global row.  Per query (one wave): the keys (dist bits << 32 | global id) of all parts
// are reduced to the knn smallest -- the global top-k, because every part's list holds its own knn smallest keys.  Only a
// query with fewer than knn keys pays for distances: slot cnt + s takes global row n_total - 1 - s, duplicates of matched
// rows included, as hvs_k_select / hvs_k_merge pad on one GPU (hvs_wave_pad), with the distance computed
// here from `tail` -- the part's replica of the last `tail_rows` rows of the whole D (tail_rows >= knn: host) -- by the engines'
// own exact-order function; pad == 0 leaves the largest key there.  `padded` counts the under-full queries either way.
// ---------------------------------------------------------------------------------------------
struct HvsPartLists {
    const uint32_t* ids[16];
    const float* dists[16];
    uint32_t row0[16];
};

template <bool SCALAR_ORDER, int CAP>
__global__ __launch_bounds__(256) void hvs_k_merge_parts(HvsPartLists parts, uint32_t nparts, uint32_t nq, const float* __restrict__ Q,
                                                         const float* __restrict__ tail, uint32_t tail_rows, uint32_t n_total, int pad,
                                                         uint32_t* __restrict__ out_ids, float* __restrict__ out_dists, uint32_t knn,
                                                         unsigned long long* __restrict__ padded)
{
    __shared__ uint64_t sbuf[4][CAP];
    __shared__ uint32_t shist[4][256];  // digit histograms of the radix select
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = threadIdx.x >> 6;
    const uint32_t q = blockIdx.x * 4u + w;
    if (q >= nq) return;  // wave-uniform
    uint64_t* buf = sbuf[w];
    uint32_t cnt = 0;
    for (uint32_t s = 0; s < nparts; ++s)
        cnt = hvs_gather_list_keys<CAP>(buf, shist[w], cnt, parts.ids[s] + (size_t)q * knn, parts.dists[s] + (size_t)q * knn, parts.row0[s], knn,
                                        lane);
    cnt = hvs_wave_final_cut<CAP>(buf, shist[w], cnt, knn, lane);
    if (cnt < knn && lane == 0u) atomicAdd(padded, 1ull);
    const float* __restrict__ qv = Q + (size_t)q * HVS_QCOLS + 4;
    hvs_wave_pad(buf, cnt, knn, pad, lane, [=](uint32_t s) {  // global row n_total - 1 - s, read from the tail replica (s < knn <= tail_rows)
        const float* __restrict__ dv = tail + (size_t)(tail_rows - 1u - s) * HVS_DCOLS + 2;
        return hvs_make_key(SCALAR_ORDER ? hvs_scalar_order_dist(dv, qv) : hvs_exact_dist(dv, qv), n_total - 1u - s);
    });
    hvs_wave_rank_write(buf, knn, lane, q, out_ids, out_dists);
}

// ---------------------------------------------------------------------------------------------
// Category sets (hvs_set_category_sets / hvs_query_in): a query of type 1 or 3 whose predicate reads "C is one of
// s_1 .. s_m" is answered as m ordinary SUB-QUERIES over the same D, one per distinct value, with padding off; rows of different
// categories are disjoint, so the k smallest keys of the union of the sub-queries' top-k lists are the set predicate's top-k.
// The engines see the expanded query set and know nothing of sets.  Host arrays (hvs_in_plan): sub_off[nq + 1] -- user query p
// owns sub-queries [sub_off[p], sub_off[p + 1]) (at least one) --, parent[nsub], value[nsub].
// ---------------------------------------------------------------------------------------------
// the engines' reading of a query's type float (hvs_parse_query): does it test C at all?
__host__ __device__ __forceinline__ bool hvs_in_type_has_c(float t)
{
    if (!(t > -1.0f && t < 4.0f)) return false;
    const uint32_t type = (uint32_t)(int32_t)t;
    return type == 1u || type == 3u;
}
// the engines' reading of a set value (reference optimized_parallel.hpp:93-96): the category its int32 truncation names, as the
// float C is compared with; false for a value that names none (NaN fails both compares, +-inf and |s| >= 2^31 one of them).  The
// result is never -0.0: equal categories have equal bits.  The host plan (hvs_in_plan) and the device plan call this one function.
__host__ __device__ __forceinline__ bool hvs_in_category(float s, float* cat)
{
    if (!(s >= -2147483648.0f && s < 2147483648.0f)) return false;
    *cat = (float)(int32_t)s;
    return true;
}

// Sub-query j = the 104 floats of user query parent[j], bit for bit, with float 1 (v) replaced by value[j] -- only where the
// parent tests C (type 1 or 3) and carries a non-empty set (set_off[p + 1] > set_off[p], the caller's CSR offsets); every
// other parent has one sub-query, itself.  One thread per float4 of a row (26 of them), consecutive threads consecutive float4s.
__global__ __launch_bounds__(256) void hvs_k_expand_in(const float4* __restrict__ Qu, const uint32_t* __restrict__ parent, const float* __restrict__ value,
                                                      const uint32_t* __restrict__ set_off, uint32_t nsub, float4* __restrict__ Qx)
{
    static_assert(HVS_QCOLS % 4u == 0u, "query rows are moved in 16-byte pieces");
    constexpr uint32_t P = HVS_QCOLS / 4u;
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (uint64_t)nsub * P) return;
    const uint32_t j = (uint32_t)(e / P), c = (uint32_t)(e - (uint64_t)j * P);
    const uint32_t p = parent[j];
    float4 v = Qu[(size_t)p * P + c];
    if (c == 0u && hvs_in_type_has_c(v.x) && set_off[p + 1u] > set_off[p]) v.y = value[j];
    Qx[e] = v;
}

// Caps and cursors stay one per USER query: sub-query j takes its parent's (the normalised forms hvs_k_norm_caps /
// hvs_k_norm_after leave).  A null input skips its output.
__global__ __launch_bounds__(256) void hvs_k_expand_per_query(const uint32_t* __restrict__ parent, uint32_t nsub, const float* __restrict__ caps_in, float* __restrict__ caps_out,
                                       const uint64_t* __restrict__ lo_in, const float* __restrict__ dist_in, const uint32_t* __restrict__ id_in,
                                       uint64_t* __restrict__ lo_out, float* __restrict__ dist_out, uint32_t* __restrict__ id_out)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nsub) return;
    const uint32_t p = parent[j];
    if (caps_in) caps_out[j] = caps_in[p];
    if (lo_in) {
        lo_out[j] = lo_in[p];
        dist_out[j] = dist_in[p];
        id_out[j] = id_in[p];
    }
}

// hvs_k_merge_in -- per user query (one wave, four per workgroup): the result rows of its sub-queries, rows [sub_off[q],
// sub_off[q + 1]) x knn of the engines' own result buffer (padding off: 0xFFFFFFFF = empty slot, ids global), are streamed
// through the wave's key buffer (hvs_gather_list_keys cuts it back to the knn smallest whenever the next 64 slots might not
// fit: that is how 64 lists pass through 256 / 512 keys) and reduced to the knn smallest keys.  The keys are distinct: the
// sub-queries' categories are (hvs_in_plan de-duplicates).  Caps and cursors were applied by the sub-queries.  Padding
// (hvs_wave_pad): slot cnt + s takes row n - 1 - s, or pad_ids[s] (the last live ids) where pad_ids is not null, with the
// distance computed here from D by the engines' own exact-order function.
// stat[0] += 1 for an under-full query, stat[1] += keys gathered.  Queries [q0, q0 + nq) of the user's set; Q: the user's rows.
template <bool SCALAR_ORDER, int CAP>
__global__ __launch_bounds__(256) void hvs_k_merge_in(const uint32_t* __restrict__ sub_off, uint32_t q0, uint32_t nq, const uint32_t* __restrict__ sub_ids,
                                                      const float* __restrict__ sub_dists, const float* __restrict__ D, uint32_t n,
                                                      const float* __restrict__ Q, int pad, const uint32_t* __restrict__ pad_ids,
                                                      uint32_t* __restrict__ out_ids, float* __restrict__ out_dists, uint32_t knn,
                                                      unsigned long long* __restrict__ stat)
{
    __shared__ uint64_t sbuf[4][CAP];
    __shared__ uint32_t shist[4][256];  // digit histograms of the radix select
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = threadIdx.x >> 6;
    const uint32_t i = blockIdx.x * 4u + w;
    if (i >= nq) return;  // wave-uniform
    const uint32_t q = q0 + i;
    uint64_t* buf = sbuf[w];
    const uint32_t s0 = sub_off[q], s1 = sub_off[q + 1u];
    uint32_t cnt = 0, seen = 0;
    for (uint32_t s = s0; s < s1; ++s) {
        const uint32_t* __restrict__ ids = sub_ids + (size_t)s * knn;
        // (hvs_in_info.merged_keys costs this second pass over the list's ids, an L2 hit: the gather may cut the buffer back in
        // mid-list, so its own count does not say what a list held)
        for (uint32_t off = 0; off < knn; off += 64u)
            seen += (uint32_t)__popcll(__ballot(off + lane < knn && ids[off + lane] != 0xFFFFFFFFu));
        cnt = hvs_gather_list_keys<CAP>(buf, shist[w], cnt, ids, sub_dists + (size_t)s * knn, 0ull, knn, lane);
    }
    cnt = hvs_wave_final_cut<CAP>(buf, shist[w], cnt, knn, lane);
    if (lane == 0u) {
        if (cnt < knn) atomicAdd(&stat[0], 1ull);
        if (seen) atomicAdd(&stat[1], (unsigned long long)seen);
    }
    const float* __restrict__ qv = Q + (size_t)q * HVS_QCOLS + 4;
    // (s < knn <= live rows: host)
    hvs_wave_pad(buf, cnt, knn, pad, lane, [=](uint32_t s) { return hvs_row_key<SCALAR_ORDER>(D, pad_ids ? pad_ids[s] : n - 1u - s, qv); });
    hvs_wave_rank_write(buf, knn, lane, q, out_ids, out_dists);
}

// ---------------------------------------------------------------------------------------------
// The plan made on the device (hvs_set_category_sets_device): what hvs_in_plan(q_rows, ...) computes, bit for bit,
// from a CSR that lies in device memory -- the set values never reach the host.  One GPU plans its `nuq` user queries from its
// slice of the offsets, off[0 .. nuq], which index the values as vals[i - v0] (v0 = 0: the caller's own array read in place;
// v0 = lo: a copy of the slice's values [lo, hi)).  Three kernels: hvs_k_in_count (one wave per query: sub-query counts and
// flags), hvs_k_in_scan (sub_off and the two 64-bit totals), and, once the host has accepted the plan, hvs_k_in_fill (one wave
// per query: parent, value and the rebased offsets hvs_k_expand_in reads).  Count and fill both build a query's distinct list:
// nothing of size nq x 64 is kept between them.
// ---------------------------------------------------------------------------------------------
#define HVS_INP_MALFORMED 1ull  // stat[0]: an offset pair that descends or leaves [lo, hi], or values missing
#define HVS_INP_TOO_MANY 2ull   // stat[0]: a set of more than HVS_IN_MAX_VALUES distinct categories
#define HVS_INP_MAX_VALUES 64u  // = HVS_IN_MAX_VALUES of the C ABI (asserted where both are seen): one lane of a wave per category

// The distinct categories of the raw values [a, b) in the order they first appear, one wave: lane j ends up holding the j-th
// in `mine` (j < the count returned; at most 64, so the list lives in the wave's registers).  The values are walked 64 at a
// time, whatever b - a is: a lane's value is dropped if it names no category or one the list has, and the rest enter the list
// leader by leader -- the lowest fresh lane appends its category and retires every lane that holds the same one.  Returns
// HVS_INP_MAX_VALUES + 1 as soon as a 65th category appears.  a, b and the result are wave-uniform.
__device__ __forceinline__ uint32_t hvs_in_distinct(const float* __restrict__ vals, uint32_t v0, uint32_t a, uint32_t b, uint32_t lane, float& mine)
{
    uint32_t n = 0;
    mine = 0.0f;
    for (uint64_t base = a; base < b; base += 64u) {  // (64 bits: b may lie within 64 of 2^32)
        const uint64_t i = base + lane;
        float cat = 0.0f;
        bool fresh = i < b && hvs_in_category(vals[(size_t)(i - v0)], &cat);
        for (uint32_t j = 0; j < n; ++j) {
            const float have = __shfl(mine, (int)j);
            if (have == cat) fresh = false;
        }
        uint64_t m = __ballot(fresh);
        while (m) {
            if (n == HVS_INP_MAX_VALUES) return HVS_INP_MAX_VALUES + 1u;
            const float lead = __shfl(cat, __ffsll((long long)m) - 1);
            if (lane == n) mine = lead;
            ++n;
            if (cat == lead) fresh = false;
            m = __ballot(fresh);
        }
    }
    return n;
}

// Count.  Query p (one wave, four per workgroup) reads its type from the user's rows Qu and its raw range [off[p], off[p + 1]);
// the range must ascend and stay inside the slice's [lo, hi] -- an ascending CSR does, and one that does not is refused before a
// value outside the caller's array could be read.  pack[p] = m | mc << 8 | eff << 16: m sub-queries (effective ?
// max(distinct, 1) : 1), mc the same under "every query tests C" (what the host call's limit is taken over), eff as
// hvs_in_plan has it.  The size limit is the set's own, whatever the query's type.  Flags are OR-ed into stat[0].
__global__ __launch_bounds__(256) void hvs_k_in_count(const float* __restrict__ Qu, const uint32_t* __restrict__ off, const float* __restrict__ vals,
                                                      uint32_t v0, uint32_t lo, uint32_t hi, uint32_t nuq, uint32_t* __restrict__ pack,
                                                      unsigned long long* __restrict__ stat)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t p = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (p >= nuq) return;  // wave-uniform
    const uint32_t a = off[p], b = off[p + 1u];
    unsigned long long flags = 0ull;
    uint32_t n = 0;
    if (!(lo <= a && a <= b && b <= hi) || (b > a && !vals)) {
        flags = HVS_INP_MALFORMED;
    } else {
        float mine;
        n = hvs_in_distinct(vals, v0, a, b, lane, mine);
        if (n > HVS_INP_MAX_VALUES) flags = HVS_INP_TOO_MANY;
    }
    if (lane == 0u) {
        const bool nonempty = !flags && b > a;
        const bool eff = nonempty && hvs_in_type_has_c(Qu[(size_t)p * HVS_QCOLS]);
        const uint32_t mc = nonempty && n > 1u ? n : 1u;
        pack[p] = (eff ? mc : 1u) | mc << 8 | (eff ? 1u : 0u) << 16;
        if (flags) atomicOr(&stat[0], flags);
    }
}

// Scan.  sub_off[0 .. nuq] = the exclusive prefix of the counts, eff[p] unpacked, stat[1] = the sub-queries, stat[2] = their
// number if every query tested C -- both sums in 64 bits (sub_off holds the low words; the host refuses what does not fit).  One
// workgroup of 1024 walks the queries in tiles of 4096, carrying the running sums, as hvs_k_item_scan is one workgroup: nothing
// waits for another workgroup, and the work is a few bytes per query.
__global__ __launch_bounds__(1024) void hvs_k_in_scan(const uint32_t* __restrict__ pack, uint32_t nuq, uint32_t* __restrict__ sub_off,
                                                      uint8_t* __restrict__ eff, unsigned long long* __restrict__ stat)
{
    __shared__ uint32_t swave[16], swave_c[16];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    unsigned long long run = 0ull, run_c = 0ull;
    for (uint64_t base = 0; base < nuq; base += 4096u) {
        const uint64_t i0 = base + threadIdx.x * 4u;
        uint32_t m[4], sum = 0, sum_c = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t pk = i0 + j < nuq ? pack[i0 + j] : 0u;
            m[j] = pk & 0xFFu;
            sum += m[j];
            sum_c += (pk >> 8) & 0xFFu;
            if (i0 + j < nuq) eff[i0 + j] = (uint8_t)((pk >> 16) & 1u);
        }
        uint32_t inc = sum;  // inclusive scan over the wave
        for (uint32_t o = 1; o < 64u; o <<= 1) {
            const uint32_t t = __shfl_up(inc, o);
            if (lane >= o) inc += t;
        }
        for (uint32_t o = 32; o; o >>= 1) sum_c += __shfl_xor(sum_c, (int)o);
        if (lane == 63u) {
            swave[w] = inc;
            swave_c[w] = sum_c;
        }
        __syncthreads();
        uint32_t before = 0, tile = 0, tile_c = 0;  // (a tile holds at most 4096 x 64 sub-queries)
        for (uint32_t x = 0; x < 16u; ++x) {
            before += x < w ? swave[x] : 0u;
            tile += swave[x];
            tile_c += swave_c[x];
        }
        __syncthreads();  // (the next tile overwrites the waves' sums)
        unsigned long long at = run + before + (inc - sum);
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j)
            if (i0 + j < nuq) {
                sub_off[i0 + j] = (uint32_t)at;
                at += m[j];
            }
        run += tile;
        run_c += tile_c;
    }
    if (threadIdx.x == 0u) {
        sub_off[nuq] = (uint32_t)run;
        stat[1] = run;
        stat[2] = run_c;
    }
}

// Fill.  Query p (one wave) writes its sub-queries [sub_off[p], sub_off[p + 1]): parent = p, and value = its own v where its
// set is not effective, else its distinct categories ascending -- rebuilt here and rank-sorted (they are distinct: the ranks
// are the places) --, or the canonical NaN where no value names a category.  set_off[0 .. nuq] = the offsets as seen from lo
// (what hvs_k_expand_in reads).  Runs on a plan the host has accepted: the ranges are good and no set is too large.
__global__ __launch_bounds__(256) void hvs_k_in_fill(const float* __restrict__ Qu, const uint32_t* __restrict__ off, const float* __restrict__ vals,
                                                     uint32_t v0, uint32_t lo, uint32_t nuq, const uint32_t* __restrict__ sub_off,
                                                     const uint8_t* __restrict__ eff, uint32_t* __restrict__ set_off, uint32_t* __restrict__ parent,
                                                     float* __restrict__ value)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t p = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (p >= nuq) return;  // wave-uniform
    const uint32_t a = off[p], b = off[p + 1u];
    const size_t s0 = sub_off[p];
    const uint32_t m = sub_off[p + 1u] - sub_off[p];
    if (lane == 0u) {
        set_off[p] = a - lo;
        if (p == nuq - 1u) set_off[nuq] = b - lo;
    }
    if (!eff[p]) {
        if (lane == 0u && m == 1u) {
            parent[s0] = p;
            value[s0] = Qu[(size_t)p * HVS_QCOLS + 1u];
        }
        return;
    }
    float mine;
    const uint32_t n = hvs_in_distinct(vals, v0, a, b, lane, mine);
    if (n == 0u) {
        if (lane == 0u && m == 1u) {
            parent[s0] = p;
            value[s0] = __uint_as_float(0x7FC00000u);
        }
        return;
    }
    if (n != m) return;  // (cannot happen: the count ran the same code on the same bytes; nothing outside the query's range is written)
    uint32_t rank = 0;
    for (uint32_t j = 0; j < n; ++j) rank += __shfl(mine, (int)j) < mine ? 1u : 0u;
    if (lane < n) {
        parent[s0 + lane] = p;
        value[s0 + rank] = mine;
    }
}

// ---------------------------------------------------------------------------------------------
// Multi-vector queries (hvs_set_query_vectors / hvs_query_vectors): user query q carries m(q) EXTRA vectors beside
// its own, given in CSR form (off[nq + 1], vecs[off[nq]][100]), and asks for the k rows with the smallest MINIMUM key over its
// 1 + m(q) vectors.  It is answered as 1 + m(q) ordinary sub-queries with padding off -- the second client of the expanded
// resident set category sets built --, and hvs_k_merge_vectors merges their lists BY ID: the sub-lists are not disjoint.
// The plan needs no scan: sub_off[q] = off[q] + q, and sub-query j of parent p reads extra vector j - p - 1 (j > sub_off[p]).
// ---------------------------------------------------------------------------------------------
#define HVS_VEC_MAX_EXTRA_ 63u  // (= HVS_VECTORS_MAX_EXTRA of include/hvs.h; hvs.hip asserts it)

// The plan of checked offsets (one GPU's slice, off[0] = lo): sub_off[q] = off[q] - lo + q, parent = q for the query's
// 1 + m(q) <= 64 sub-queries.  One thread per user query (thread nq writes the last offset).
__global__ void hvs_k_fill_vectors(const uint32_t* __restrict__ off, uint32_t nq, uint32_t* __restrict__ sub_off, uint32_t* __restrict__ parent)
{
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q > nq) return;
    const uint32_t lo = off[0];
    const uint32_t s0 = off[q] - lo + q;
    sub_off[q] = s0;
    if (q == nq) return;
    uint32_t m = off[q + 1u] - off[q];
    if (m > HVS_VEC_MAX_EXTRA_) m = HVS_VEC_MAX_EXTRA_;  // (refused by the host before this launch; never trusted here)
    for (uint32_t j = 0; j <= m; ++j) parent[s0 + j] = q;
}

// Sub-query j = the 26 float4s of user query parent[j]; float4s 1..25 (the vector) come from extra vector j - p - 1 of `vecs`
// (this GPU's slice of the extras, 25 float4s each) when j is not the parent's first sub-query.  One thread per float4,
// consecutive threads consecutive float4s, like hvs_k_expand_in.
__global__ __launch_bounds__(256) void hvs_k_expand_vectors(const float4* __restrict__ Qu, const uint32_t* __restrict__ parent,
                                                           const uint32_t* __restrict__ sub_off, const float4* __restrict__ vecs, uint32_t nsub,
                                                           float4* __restrict__ Qx)
{
    static_assert(HVS_QCOLS % 4u == 0u && HVS_NDIM % 4u == 0u && HVS_QCOLS == HVS_NDIM + 4u, "rows are moved in 16-byte pieces");
    constexpr uint32_t P = HVS_QCOLS / 4u, V = HVS_NDIM / 4u;
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (uint64_t)nsub * P) return;
    const uint32_t j = (uint32_t)(e / P), c = (uint32_t)(e - (uint64_t)j * P);
    const uint32_t p = parent[j];
    const bool own = c == 0u || j == sub_off[p];
    Qx[e] = own ? Qu[(size_t)p * P + c] : vecs[(size_t)(j - p - 1u) * V + (c - 1u)];
}

// The wave's key buffer buf[0 .. cnt) de-duplicated BY ID, in place: per id the smallest key stays, and one of two equal
// keys.  How: the keys are rotated to (id << 32 | distance bits) and sorted by a bitonic network over the next power of two
// >= 64 (the tail filled with ~0, which no key is: an id of 0xFFFFFFFF names no row) -- equal ids are then neighbours, the
// smallest distance first --, and the first of every run is kept by a ballot compaction that rotates it back.  P log2(P)
// (log2(P) + 1) / 4 compare-exchanges over 64 lanes: 36 rounds of 2 per lane at P = 256, 45 of 4 at P = 512 (an all-pairs
// scan would read P keys per key: 1024 / 4096 LDS reads per lane).  The buffer is left in id order, which the radix select
// and the rank sort behind it do not mind.  Returns the keys left.  Wave-uniform: all 64 lanes call it.
template <int CAP>
__device__ __forceinline__ uint32_t hvs_wave_dedup_ids(uint64_t* buf, uint32_t cnt, uint32_t lane)
{
    uint32_t P = 64u;
    while (P < cnt) P <<= 1;  // (cnt <= CAP, a power of two: P <= CAP)
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    for (uint32_t e = lane; e < P; e += 64u) {
        const uint64_t k = e < cnt ? buf[e] : ~0ull;
        buf[e] = (k << 32) | (k >> 32);
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    for (uint32_t k = 2u; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
            for (uint32_t i = lane; i < P; i += 64u) {
                const uint32_t l = i ^ j;
                if (l > i) {
                    const uint64_t a = buf[i], b = buf[l];
                    if ((a > b) == ((i & k) == 0u)) {
                        buf[i] = b;
                        buf[l] = a;
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        }
    }
    uint32_t kept = 0;
    uint32_t prev_id = 0xFFFFFFFFu;  // id in front of the chunk (no key has it: the first entry is always kept)
    for (uint32_t off = 0; off < cnt; off += 64u) {  // (wave-uniform; a chunk's keys land at or below their own places)
        const uint32_t e = off + lane;
        const uint64_t r = e < cnt ? buf[e] : ~0ull;
        const uint32_t id = (uint32_t)(r >> 32);
        const uint32_t left = (uint32_t)__shfl_up((int)id, 1);
        const uint32_t before = lane == 0u ? prev_id : left;
        prev_id = (uint32_t)__shfl((int)id, 63);  // (read before this chunk's stores may overwrite the entry)
        const bool in = e < cnt && id != before;
        const uint64_t m = __ballot(in);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        if (in) buf[kept + hvs_prefix_count(m)] = (r << 32) | (r >> 32);
        kept += (uint32_t)__popcll(m);
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    return kept;
}

// hvs_k_merge_vectors -- per user query (one wave, four per workgroup): the result rows of its 1 + m sub-queries, rows
// [sub_off[q], sub_off[q + 1]) x knn of the engines' result buffer (padding off: 0xFFFFFFFF = empty slot, ids global), are
// streamed through the wave's key buffer, 64 slots at a time.  The same row turns up in several lists with different keys, so
// this is not hvs_k_merge_in: whenever the next 64 slots might not fit (held + 64 > CAP) the buffer is first DE-DUPLICATED by id
// (hvs_wave_dedup_ids), and only if they still might not fit cut back to its knn smallest keys
// -- a cut over duplicates could keep two keys of one row and drop a row the answer needs; after de-duplication a dropped row
// has knn distinct rows in front of it, whose keys only shrink as more lists arrive, and a later, smaller key of the dropped
// row is gathered again.  knn + 64 <= CAP, so the step then fits.  Once more at the end: de-duplicate, then select -- the keys
// are distinct whenever hvs_wave_select_prune runs, the exact duplicate (equal vectors) included.  Caps and exclusion lists
// were applied by the sub-queries.  Padding as hvs_k_merge_in: slot cnt + s takes row n - 1 - s or pad_ids[s], with the
// smallest key over the query's vectors, read from the EXPANDED rows Qx[sub_off[q] .. sub_off[q + 1]) (hvs_row_key_min).
// stat[0] += 1 for an under-full query, stat[1] += keys read, stat[2] += keys dropped because the buffer held the id with a key
// at least as small.  Queries [q0, q0 + nq) of the user's set.
template <bool SCALAR_ORDER, int CAP>
__global__ __launch_bounds__(256) void hvs_k_merge_vectors(const uint32_t* __restrict__ sub_off, uint32_t q0, uint32_t nq, const uint32_t* __restrict__ sub_ids,
                                                           const float* __restrict__ sub_dists, const float* __restrict__ D, uint32_t n,
                                                           const float* __restrict__ Qx, int pad, const uint32_t* __restrict__ pad_ids,
                                                           uint32_t* __restrict__ out_ids, float* __restrict__ out_dists, uint32_t knn,
                                                           unsigned long long* __restrict__ stat)
{
    __shared__ uint64_t sbuf[4][CAP];
    __shared__ uint32_t shist[4][256];  // digit histograms of the radix select
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = threadIdx.x >> 6;
    const uint32_t i = blockIdx.x * 4u + w;
    if (i >= nq) return;  // wave-uniform; waves never meet at a barrier
    const uint32_t q = q0 + i;
    uint64_t* buf = sbuf[w];
    const uint32_t s0 = sub_off[q], s1 = sub_off[q + 1u];
    uint32_t cnt = 0, seen = 0, dups = 0;
    for (uint32_t s = s0; s < s1; ++s) {
        const uint32_t* __restrict__ ids = sub_ids + (size_t)s * knn;
        const float* __restrict__ dists = sub_dists + (size_t)s * knn;
        for (uint32_t off = 0; off < knn; off += 64u) {
            if (cnt + 64u > (uint32_t)CAP) {
                const uint32_t left = hvs_wave_dedup_ids<CAP>(buf, cnt, lane);
                dups += cnt - left;
                cnt = left;
                if (cnt + 64u > (uint32_t)CAP) {  // (cnt > knn: knn + 64 <= CAP)
                    hvs_wave_select_prune<CAP / 64>(buf, cnt, knn, lane, shist[w]);
                    cnt = knn;
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                }
            }
            const uint32_t e = off + lane;
            const uint32_t id = e < knn ? ids[e] : 0xFFFFFFFFu;
            const bool have = id != 0xFFFFFFFFu;
            const uint64_t m = __ballot(have);
            if (have) buf[cnt + hvs_prefix_count(m)] = hvs_make_key(dists[e], id);
            cnt += (uint32_t)__popcll(m);
            seen += (uint32_t)__popcll(m);
        }
    }
    if (s1 - s0 > 1u) {  // (one list holds every id once)
        const uint32_t left = hvs_wave_dedup_ids<CAP>(buf, cnt, lane);
        dups += cnt - left;
        cnt = left;
    }
    cnt = hvs_wave_final_cut<CAP>(buf, shist[w], cnt, knn, lane);
    if (lane == 0u) {
        if (cnt < knn) atomicAdd(&stat[0], 1ull);
        if (seen) atomicAdd(&stat[1], (unsigned long long)seen);
        if (dups) atomicAdd(&stat[2], (unsigned long long)dups);
    }
    // (s < knn <= live rows: host)
    hvs_wave_pad(buf, cnt, knn, pad, lane, [=](uint32_t s) { return hvs_row_key_min<SCALAR_ORDER>(D, pad_ids ? pad_ids[s] : n - 1u - s, Qx, s0, s1); });
    hvs_wave_rank_write(buf, knn, lane, q, out_ids, out_dists);
}

// ---------------------------------------------------------------------------------------------
// Query clauses (hvs_set_query_clauses / hvs_query_clauses): user query q carries m(q) EXTRA clauses beside its own
// row, in CSR form (off[nq + 1], attrs[off[nq]][4] = [type, v, l, r], and optionally vecs[off[nq]][100]), and asks for the k
// rows with the smallest MINIMUM key over the clauses they pass.  It is answered as 1 + m(q) <= 256 ordinary sub-queries with
// padding off -- the third client of the expanded resident set --, and hvs_k_merge_clauses merges their lists by id.  The plan is
// that of the extra vectors: sub_off[q] = off[q] + q, and sub-query j of parent p reads extra clause j - p - 1 (j > sub_off[p]).
// ---------------------------------------------------------------------------------------------
#define HVS_CLAUSE_MAX_EXTRA_ 255u  // (= HVS_CLAUSES_MAX_EXTRA of include/hvs.h; hvs.hip asserts it)

// The plan of checked offsets (one GPU's slice, off[0] = lo): sub_off[q] = off[q] - lo + q, parent = q for the query's
// 1 + m(q) <= 256 sub-queries.  One WAVE per user query (four per workgroup; wave nq writes the last offset): a thread per query,
// as hvs_k_fill_vectors has it, would write up to 256 scattered words; a thread per sub-query would have to search sub_off, which
// this very kernel writes, so it would take a second launch.  A wave needs neither: its 64 lanes store the parent's index to
// consecutive words, four stores at the most.
__global__ __launch_bounds__(256) void hvs_k_fill_clauses(const uint32_t* __restrict__ off, uint32_t nq, uint32_t* __restrict__ sub_off,
                                                         uint32_t* __restrict__ parent)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (q > nq) return;  // wave-uniform
    const uint32_t lo = off[0];
    const uint32_t s0 = off[q] - lo + q;
    if (lane == 0u) sub_off[q] = s0;
    if (q == nq) return;
    uint32_t m = off[q + 1u] - off[q];
    if (m > HVS_CLAUSE_MAX_EXTRA_) m = HVS_CLAUSE_MAX_EXTRA_;  // (refused by the host before this launch; never trusted here)
    for (uint32_t j = lane; j <= m; j += 64u) parent[s0 + j] = q;
}

// Sub-query j = 26 float4s.  Float4 0 ([type, v, l, r]) is the parent's for the parent's first sub-query, else extra clause
// j - p - 1 of `attrs`; float4s 1..25 (the vector) are the parent's for its first sub-query and whenever `vecs` is null
// (predicate-only clauses), else extra vector j - p - 1 of `vecs` (25 float4s each).  attrs and vecs: this GPU's slice of the
// extras.  One thread per float4, consecutive threads consecutive float4s, like hvs_k_expand_vectors.
__global__ __launch_bounds__(256) void hvs_k_expand_clauses(const float4* __restrict__ Qu, const uint32_t* __restrict__ parent,
                                                           const uint32_t* __restrict__ sub_off, const float4* __restrict__ attrs,
                                                           const float4* __restrict__ vecs, uint32_t nsub, float4* __restrict__ Qx)
{
    static_assert(HVS_QCOLS % 4u == 0u && HVS_NDIM % 4u == 0u && HVS_QCOLS == HVS_NDIM + 4u, "rows are moved in 16-byte pieces");
    constexpr uint32_t P = HVS_QCOLS / 4u, V = HVS_NDIM / 4u;
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (uint64_t)nsub * P) return;
    const uint32_t j = (uint32_t)(e / P), c = (uint32_t)(e - (uint64_t)j * P);
    const uint32_t p = parent[j];
    const bool first = j == sub_off[p];
    float4 v;
    if (c == 0u)
        v = first ? Qu[(size_t)p * P] : attrs[j - p - 1u];
    else
        v = first || !vecs ? Qu[(size_t)p * P + c] : vecs[(size_t)(j - p - 1u) * V + (c - 1u)];
    Qx[e] = v;
}

// hvs_k_merge_clauses -- hvs_k_merge_vectors for up to 256 lists per user query (one wave, four per workgroup): the result rows
// of its sub-queries, rows [sub_off[q], sub_off[q + 1]) x knn of the engines' result buffer (padding off: 0xFFFFFFFF = empty slot,
// ids global), are streamed in sub-query order through the wave's key buffer, 64 slots at a time; the buffer is de-duplicated
// by id (hvs_wave_dedup_ids) before any cut and once more before the final select, exactly as there, and for the reasons given
// there.  What is new is a wave-uniform THRESHOLD tau, "no key" (~0, which no key is) to begin with, under this invariant:
//     whenever tau is set, the buffer holds knn distinct ids whose keys are <= tau.
// Every cut (hvs_wave_select_prune to knn after a de-duplication) sets tau to the largest key kept, which establishes it.  A
// loaded key is admitted only if it is STRICTLY below tau; a key equal to tau is the very entry held (a key names its id).
// That keeps the invariant -- the knn rows behind tau stay in the buffer until a cut, a de-duplication only replaces a key by a
// smaller one of the same id, and a cut over >= knn distinct ids with keys <= tau yields a tau no larger -- and it loses
// nothing: a row whose smallest key is >= tau has knn other rows in front of it now and for ever, since their keys only shrink;
// a row of the answer, whose smallest key is below every tau there ever is, is admitted whenever that key arrives.
// Sub-lists ascend in key order, non-finite distances behind the finite ones and empty slots last, so once a chunk held a slot
// that was empty or not below tau, nothing further in that list can be admitted: its remaining chunks are not loaded (tau only
// falls).  tau lives in scalar registers (hvs_wave_select_prune returns it wave-uniform), and the admission test is part of
// the ballot that compacts the chunk.  No LDS beyond the key buffer and the select's histogram.
// Padding and the final rank sort are hvs_k_merge_vectors': a pad row's key is its smallest over the query's EXPANDED rows.
// (With predicate-only clauses these rows all carry the parent's vector, and a pad slot computes the same distance up to 256
// times: the kernel is not told which kind it merges.  That costs only under-full queries with padding on.)  From the final cut
// on, the text is what hvs_wave_final_cut, hvs_wave_pad with hvs_row_key_min and hvs_wave_rank_write hold (hvs_device.h),
// written out: with the calls this kernel's code came out 17 to 21 instructions shorter and, in one of the six timings that
// run it, 0.001 ms outside the old code's range on the slow side (profiles/merge_tail_rate.txt).  A fix to the tail goes here too.
// stat[0] += 1 for an under-full query, stat[1] += non-empty slots loaded, stat[2] += keys dropped by a de-duplication,
// stat[3] += keys loaded and not admitted, stat[4] += 64-slot chunks never loaded.  Queries [q0, q0 + nq) of the user's set.
template <bool SCALAR_ORDER, int CAP>
__global__ __launch_bounds__(256) void hvs_k_merge_clauses(const uint32_t* __restrict__ sub_off, uint32_t q0, uint32_t nq, const uint32_t* __restrict__ sub_ids,
                                                           const float* __restrict__ sub_dists, const float* __restrict__ D, uint32_t n,
                                                           const float* __restrict__ Qx, int pad, const uint32_t* __restrict__ pad_ids,
                                                           uint32_t* __restrict__ out_ids, float* __restrict__ out_dists, uint32_t knn,
                                                           unsigned long long* __restrict__ stat)
{
    __shared__ uint64_t sbuf[4][CAP];
    __shared__ uint32_t shist[4][256];  // digit histograms of the radix select
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = threadIdx.x >> 6;
    const uint32_t i = blockIdx.x * 4u + w;
    if (i >= nq) return;  // wave-uniform; waves never meet at a barrier
    const uint32_t q = q0 + i;
    uint64_t* buf = sbuf[w];
    const uint32_t s0 = sub_off[q], s1 = sub_off[q + 1u];
    const uint32_t chunks = (knn + 63u) / 64u;
    uint64_t tau = ~0ull;
    uint32_t cnt = 0, seen = 0, dups = 0, bounded = 0, skipped = 0;
    for (uint32_t s = s0; s < s1; ++s) {
        const uint32_t* __restrict__ ids = sub_ids + (size_t)s * knn;
        const float* __restrict__ dists = sub_dists + (size_t)s * knn;
        for (uint32_t ch = 0; ch < chunks; ++ch) {
            if (cnt + 64u > (uint32_t)CAP) {
                const uint32_t left = hvs_wave_dedup_ids<CAP>(buf, cnt, lane);
                dups += cnt - left;
                cnt = left;
                if (cnt + 64u > (uint32_t)CAP) {  // (cnt > knn: knn + 64 <= CAP)
                    const uint64_t kth = hvs_wave_select_prune<CAP / 64>(buf, cnt, knn, lane, shist[w]);
                    tau = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(kth >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)kth);
                    cnt = knn;
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                }
            }
            const uint32_t e = ch * 64u + lane;
            const bool slot = e < knn;
            const uint32_t id = slot ? ids[e] : 0xFFFFFFFFu;
            const bool have = id != 0xFFFFFFFFu;
            const uint64_t key = have ? hvs_make_key(dists[e], id) : ~0ull;
            const bool admit = key < tau;  // (false for an empty slot: tau <= ~0)
            const uint64_t hm = __ballot(have), m = __ballot(admit);
            if (admit) buf[cnt + hvs_prefix_count(m)] = key;
            cnt += (uint32_t)__popcll(m);
            seen += (uint32_t)__popcll(hm);
            bounded += (uint32_t)__popcll(hm & ~m);
            if (m != __ballot(slot)) {  // (a slot of the chunk was empty or not below tau: so is everything behind it)
                skipped += chunks - 1u - ch;
                break;
            }
        }
    }
    if (s1 - s0 > 1u) {  // (one list holds every id once)
        const uint32_t left = hvs_wave_dedup_ids<CAP>(buf, cnt, lane);
        dups += cnt - left;
        cnt = left;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    if (cnt > knn) {
        hvs_wave_select_prune<CAP / 64>(buf, cnt, knn, lane, shist[w]);
        cnt = knn;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    }
    if (lane == 0u) {
        if (cnt < knn) atomicAdd(&stat[0], 1ull);
        if (seen) atomicAdd(&stat[1], (unsigned long long)seen);
        if (dups) atomicAdd(&stat[2], (unsigned long long)dups);
        if (bounded) atomicAdd(&stat[3], (unsigned long long)bounded);
        if (skipped) atomicAdd(&stat[4], (unsigned long long)skipped);
    }
    for (uint32_t base = cnt; base < knn; base += 64u) {
        const uint32_t e = base + lane;
        if (e < knn) {
            uint64_t key = ~0ull;
            if (pad) {
                const uint32_t s = e - cnt;  // (< knn <= live rows: host)
                const uint32_t id = pad_ids ? pad_ids[s] : n - 1u - s;
                const float* __restrict__ dv = D + (size_t)id * HVS_DCOLS + 2;
                for (uint32_t j = s0; j < s1; ++j) {
                    const float* __restrict__ qv = Qx + (size_t)j * HVS_QCOLS + 4;
                    const uint64_t kj = hvs_make_key(SCALAR_ORDER ? hvs_scalar_order_dist(dv, qv) : hvs_exact_dist(dv, qv), id);
                    key = kj < key ? kj : key;
                }
            }
            buf[e] = key;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    // rank sort of exactly knn keys (duplicates possible after padding: ties broken by slot)
    for (uint32_t e = lane; e < knn; e += 64u) {
        const uint64_t ke = buf[e];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < knn; ++j) {
            const uint64_t kj = buf[j];
            rank += (kj < ke || (kj == ke && j < e)) ? 1u : 0u;
        }
        out_ids[(size_t)q * knn + rank] = hvs_key_id(ke);
        if (out_dists) out_dists[(size_t)q * knn + rank] = ke == ~0ull ? __builtin_inff() : hvs_key_dist(ke);
    }
}

// ---------------------------------------------------------------------------------------------
// Per-query candidate lists (hvs_set_candidate_ids / hvs_query_among): a set of row ids per resident query; a row
// takes part in the query's answer only if its id IS in the set.  The mirror image of the exclusion lists above, and attached
// the same way: the caller's CSR is put on the device as it is, hvs_k_check_offsets looks at the offsets, the host reads the
// status block back and refuses before anything changes, then hvs_k_norm_candidates normalises every list IN PLACE by the rule
// of hvs_k_norm_exclude (hvs_exclude_keeps for the part's window, minus row0, ascending, no duplicates, the rest of the raw
// extent 0xFFFFFFFF) -- what hvs_candidates_plan does on the host, bit for bit.
// No engine answers such a query: the lists are short against D, so hvs_k_scan_candidates gathers the listed rows by id.
// ---------------------------------------------------------------------------------------------
#define HVS_CANDIDATES_MAX_ 8192u  // (= HVS_CANDIDATES_MAX of include/hvs.h; hvs.hip asserts it)
// One workgroup per query, the list in LDS (32 KB): a bitonic network over the next power of two >= 256, every thread of the
// block on the same list (so the barriers are uniform); the first wave then keeps the first of every run of equal ids by a
// ballot compaction and writes them back over the raw list.  The offsets were checked: len <= 8192.
__global__ __launch_bounds__(256) void hvs_k_norm_candidates(const uint32_t* __restrict__ off, uint32_t nq, uint32_t* __restrict__ ids,
                                                             uint32_t row0, uint32_t n_rows, uint32_t* __restrict__ begin,
                                                             uint32_t* __restrict__ count)
{
    __shared__ uint32_t s[HVS_CANDIDATES_MAX_];
    const uint32_t q = blockIdx.x, t = threadIdx.x;
    if (q >= nq) return;  // block-uniform
    const uint32_t base = off[q] - off[0];
    uint32_t len = off[q + 1u] - off[q];
    if (len > HVS_CANDIDATES_MAX_) len = HVS_CANDIDATES_MAX_;  // (refused by the host before this launch; never trusted here)
    uint32_t* __restrict__ mine = ids + base;
    uint32_t P = 256u;
    while (P < len) P <<= 1;
    for (uint32_t e = t; e < P; e += 256u) {
        const uint32_t id = e < len ? mine[e] : 0xFFFFFFFFu;
        s[e] = hvs_exclude_keeps(id, row0, n_rows) ? id - row0 : 0xFFFFFFFFu;
    }
    __syncthreads();
    for (uint32_t k = 2u; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
            for (uint32_t i = t; i < P; i += 256u) {
                const uint32_t l = i ^ j;
                if (l > i) {
                    const uint32_t a = s[i], b = s[l];
                    if ((a > b) == ((i & k) == 0u)) {
                        s[i] = b;
                        s[l] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    if (t >= 64u) return;  // (no barrier behind this line)
    uint32_t kept = 0;
    for (uint32_t off0 = 0; off0 < len; off0 += 64u) {  // (wave-uniform; s[e] for e >= len is 0xFFFFFFFF after the sort)
        const uint32_t e = off0 + t;
        const uint32_t id = e < len ? s[e] : 0xFFFFFFFFu;
        const bool in = id != 0xFFFFFFFFu && (e == 0u || s[e - 1u] != id);
        const uint64_t m = __ballot(in);
        if (in) mine[kept + hvs_prefix_count(m)] = id;
        kept += (uint32_t)__popcll(m);
    }
    for (uint32_t e = kept + t; e < len; e += 64u) mine[e] = 0xFFFFFFFFu;
    if (t == 0u) {
        begin[q] = base;
        count[q] = kept;
    }
}

// ---------------------------------------------------------------------------------------------
// hvs_k_scan_candidates -- the whole answer of a query that carries a candidate list, one wave per query, four per
// workgroup, written straight into the resident result rows.  The list is normalised: ascending, distinct, ids of this GPU's
// rows.  A step takes ROWS listed ids.
//   SIMD order: ROWS = 16, four lanes per row, the arithmetic of hvs_exact_dist_pk dealt out over the quad: lane t plays
//     accumulators 2t, 2t+1 as one packed f32 pair -- dims (8b + 2t, 8b + 2t + 1) of the twelve full steps, and for t >= 2 dims
//     96 + 2(t - 2), + 1 of the masked tail --, then (a0+a4, a1+a5) and (a2+a6, a3+a7) by an exchange with lane t ^ 2, the sum of
//     the pair's halves, and a + b2 by an exchange with lane t ^ 1.  Every operation is the one hvs_exact_dist performs on the same
//     operands (an f32 add commutes), so the bits are its bits.  A load instruction reads 16 rows x 32 contiguous bytes, and the
//     four instructions of one 128-byte line follow each other.
//   Scalar order: one dependent chain of 100 adds, so ROWS = 64, one lane per row, each lane reading its own row
//     (hvs_scalar_order_dist, the very text the other exact kernels run).
// The loop is software-pipelined two deep: while step i computes, the attributes C, T of step i + 1 and the ids of step i + 2
// are in flight, so of the dependent chain id -> C, T -> vector only the vector's load is ever waited for.
// Per row, in this order: `id < sn` (the sampled prefix, the row cut of a part, and what keeps every id inside D), the live bit
// (`live` != nullptr: a mask is set), then C and T through hvs_row_passes.  A step in which no row passes computes no distance.
// Per key, in this order: the cap (`caps`), the cursor (`after_lo`), the wave-uniform threshold tau, and the query's exclusion
// list last (`excl.begin`; each != nullptr while attached): a listed row costs no binary search until everything else admits it.
// Keys go to the wave's LDS buffer by ballot compaction; when the next step might not fit, hvs_wave_select_prune cuts to knn and
// tau becomes the largest key kept.  The invariant is hvs_k_merge_clauses': whenever tau is set the buffer holds knn admitted
// keys <= tau, and only keys strictly below tau are admitted; the keys are distinct because the ids are, so nothing is
// de-duplicated.  A key that is refused has knn admitted keys in front of it, now and for ever.
// The end of a query is the merge family's: hvs_wave_final_cut, padding from D (or `pad_ids` under a mask), hvs_wave_rank_write.
// counters: HVS_CNT_PAIRS += listed rows that are in the prefix, live and pass the predicate; HVS_CNT_SCANNED += entries of the
// normalised list; HVS_CNT_CAND_SLOTS += slots kept; HVS_CNT_CAND_UNDERFULL += 1 for an under-full query; and the slots /
// under-full pairs of caps, cursors and exclusion lists where those are attached, as the final kernels count them.
// A wave owns a whole list: a call of few queries with long lists runs as long as its longest wave.
// ---------------------------------------------------------------------------------------------
template <bool SCALAR_ORDER, int CAP>
__global__ __launch_bounds__(256) void hvs_k_scan_candidates(const float* __restrict__ D, uint32_t n, uint32_t sn, const float* __restrict__ Q,
                                                             uint32_t q0, uint32_t nq, HvsExcl cand, const uint32_t* __restrict__ live,
                                                             const float* __restrict__ caps, const uint64_t* __restrict__ after_lo,
                                                             HvsExcl excl, int pad, const uint32_t* __restrict__ pad_ids,
                                                             uint32_t* __restrict__ out_ids, float* __restrict__ out_dists, uint32_t knn,
                                                             unsigned long long* __restrict__ counters)
{
    constexpr uint32_t ROWS = SCALAR_ORDER ? 64u : 16u;  // rows per step
    constexpr uint32_t LPR = 64u / ROWS;                 // lanes per row
    __shared__ uint64_t sbuf[4][CAP];
    __shared__ uint32_t shist[4][256];  // digit histograms of the radix select
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = threadIdx.x >> 6;
    const uint32_t i = blockIdx.x * 4u + w;
    if (i >= nq) return;  // wave-uniform; waves never meet at a barrier
    const uint32_t q = q0 + i;
    uint64_t* buf = sbuf[w];
    const HvsQParams p = hvs_parse_query(Q + (size_t)q * HVS_QCOLS);
    const float* __restrict__ qv = Q + (size_t)q * HVS_QCOLS + 4;
    const uint32_t* __restrict__ lst = cand.ids + cand.begin[q];
    const uint32_t len = cand.count[q];
    const float cap = caps ? caps[q] : 0.0f;
    const uint64_t key_lo = after_lo ? after_lo[q] : 0ull;
    const uint32_t* __restrict__ xl = excl.begin ? excl.ids + excl.begin[q] : nullptr;
    const uint32_t xn = excl.begin ? excl.count[q] : 0u;
    const uint32_t r = lane / LPR, t = lane % LPR;  // this lane's row of a step, and its place among the row's lanes
    const bool first = t == 0u;                     // the lane that speaks for its row
    hvs_f2 q2[13];                                  // (SIMD order) the query's pairs this lane's accumulators meet
    if constexpr (!SCALAR_ORDER) {
#pragma unroll
        for (int b = 0; b < 12; ++b) q2[b] = *reinterpret_cast<const hvs_f2*>(qv + 8 * b + 2 * t);
        q2[12] = t >= 2u ? *reinterpret_cast<const hvs_f2*>(qv + 96 + 2 * (t - 2u)) : hvs_f2{0.0f, 0.0f};
    }
    uint64_t tau = ~0ull;
    uint32_t cnt = 0, npass = 0, nset = 0;  // (nset: keys refused by the query's row set)
    // the pipeline's two stages in front of the step: ids of the step after the next, id and attributes of the next
    auto load_id = [&](uint32_t e) -> uint32_t { return e < len ? lst[e] : 0xFFFFFFFFu; };
    auto load_ct = [&](uint32_t id) -> float2 {  // (`id < sn` keeps the address inside D; 0xFFFFFFFF is no row: sn <= n)
        return id < sn ? *reinterpret_cast<const float2*>(D + (size_t)id * HVS_DCOLS) : float2{0.0f, 0.0f};
    };
    uint32_t id_a = load_id(r), id_b = load_id(ROWS + r);
    float2 ct_a = load_ct(id_a);
    for (uint32_t base = 0; base < len; base += ROWS) {  // wave-uniform
        const uint32_t id = id_a;
        const float2 ct = ct_a;
        id_a = id_b;
        ct_a = load_ct(id_a);
        id_b = load_id(base + 2u * ROWS + r);
        bool ok = id < sn;
        if (live != nullptr && ok) ok = hvs_row_live(live, id);
        ok = ok && hvs_row_passes(p, ct.x, ct.y);
        const uint64_t pm = __ballot(ok && first);
        if (pm == 0ull) continue;
        npass += (uint32_t)__popcll(pm);
        cnt = hvs_wave_make_room<CAP>(buf, shist[w], cnt, ROWS, knn, lane, &tau);  // (a cut sets tau; knn + 64 <= CAP)
        const float* __restrict__ dv = D + (size_t)(ok ? id : 0u) * HVS_DCOLS + 2;
        float dist = 0.0f;
        if constexpr (SCALAR_ORDER) {
            if (ok) dist = hvs_scalar_order_dist(dv, qv);
        } else {
            hvs_f2 acc = hvs_f2{0.0f, 0.0f};
            if (ok) {  // (the same for the four lanes of a row)
                const hvs_f2* __restrict__ d2 = reinterpret_cast<const hvs_f2*>(dv);  // (8-byte aligned: 408 id + 8)
#pragma unroll
                for (int b = 0; b < 12; ++b) {
                    hvs_f2 x = d2[4 * b + t] - q2[b];
                    x = x * x;
                    acc = acc + x;
                }
                if (t >= 2u) {  // the masked tail: dims 96..99 into accumulators 4..7
                    hvs_f2 x = d2[46u + t] - q2[12];
                    x = x * x;
                    acc = acc + x;
                }
            }
            hvs_f2 s;  // (a0+a4, a1+a5) on lanes 0 and 2, (a2+a6, a3+a7) on lanes 1 and 3
            s.x = acc.x + __shfl_xor(acc.x, 2);
            s.y = acc.y + __shfl_xor(acc.y, 2);
            const float h = s.x + s.y;
            dist = h + __shfl_xor(h, 1);
        }
        bool admit = false;
        uint64_t key = ~0ull;
        if (ok && first) {
            key = hvs_make_key(dist, id);
            admit = true;
            if (caps != nullptr) admit = dist <= cap;
            admit = admit && key >= key_lo && key < tau;
            if (admit && xl != nullptr) admit = !hvs_excluded(xl, xn, id);
            if (admit && !hvs_in_row_set(excl, q, id)) admit = false, ++nset;
        }
        const uint64_t m = __ballot(admit);
        if (admit) buf[cnt + hvs_prefix_count(m)] = key;
        cnt += (uint32_t)__popcll(m);
    }
    cnt = hvs_wave_final_cut<CAP>(buf, shist[w], cnt, knn, lane);
    if (excl.set_of != nullptr) {  // (wave-uniform)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nset += __shfl_xor(nset, o);
    }
    if (lane == 0u) {
        const unsigned long long under = cnt < knn ? 1ull : 0ull;
        if (excl.set_of != nullptr) {
            if (cnt) atomicAdd(&counters[HVS_CNT_SET_SLOTS], (unsigned long long)cnt);
            if (under) atomicAdd(&counters[HVS_CNT_SET_UNDERFULL], under);
            if (excl.set_of[q] != 0xFFFFFFFFu) atomicAdd(&counters[HVS_CNT_SET_RESTRICTED], 1ull);
            if (nset) atomicAdd(&counters[HVS_CNT_SET_REFUSED], (unsigned long long)nset);
        }
        if (npass) atomicAdd(&counters[HVS_CNT_PAIRS], (unsigned long long)npass);
        if (len) atomicAdd(&counters[HVS_CNT_SCANNED], (unsigned long long)len);
        if (cnt) atomicAdd(&counters[HVS_CNT_CAND_SLOTS], (unsigned long long)cnt);
        if (under) atomicAdd(&counters[HVS_CNT_CAND_UNDERFULL], under);
        if (caps != nullptr) {
            if (cnt) atomicAdd(&counters[HVS_CNT_WITHIN_SLOTS], (unsigned long long)cnt);
            if (under) atomicAdd(&counters[HVS_CNT_WITHIN_UNDERFULL], under);
        }
        if (after_lo != nullptr) {
            if (cnt) atomicAdd(&counters[HVS_CNT_AFTER_SLOTS], (unsigned long long)cnt);
            if (under) atomicAdd(&counters[HVS_CNT_AFTER_UNDERFULL], under);
        }
        if (excl.begin != nullptr) {
            if (cnt) atomicAdd(&counters[HVS_CNT_EXCL_SLOTS], (unsigned long long)cnt);
            if (under) atomicAdd(&counters[HVS_CNT_EXCL_UNDERFULL], under);
        }
    }
    // fewer than knn admitted rows (s < knn <= live rows: host)
    hvs_wave_pad(buf, cnt, knn, pad, lane, [=](uint32_t s) { return hvs_row_key<SCALAR_ORDER>(D, pad_ids ? pad_ids[s] : n - 1u - s, qv); });
    hvs_wave_rank_write(buf, knn, lane, q, out_ids, out_dists);
}
