// hvs_device.h -- device-side building blocks shared by the gfx950 kernels.
//
// Everything here must reproduce the reference's float32 results bit for bit, so this
// translation unit is built with -ffp-contract=off (hipcc contracts a + b*b into v_fmac_f32
// by default; the reference is built without FMA, CMakeLists.txt:8).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#define HVS_DCOLS 102
#define HVS_QCOLS 104
#define HVS_NDIM 100
#define HVS_KNN 100     // default k (the reference's KNN_LIMIT, optimized_impl.h:26); hvs_set_k changes it per context
#define HVS_KMAX 256    // largest k: lists of 64 NK keys with NK = 4 (k <= 128) or 8 (k <= 256)
#define HVS_WAVE 64

// ---------------------------------------------------------------------------------------------
// The per-call device counters (u64 each; host side: HvsCallState::d_counters, DESIGN 3.5a has the table of writers and
// readers).  Kernels add to `counters[slot]`, the host reads runs of slots by the same names.  The numbers are fixed: a slot
// that nothing uses is a gap, never re-used by renumbering.
// ---------------------------------------------------------------------------------------------
enum HvsCounter : int {
    HVS_CNT_PAIRS = 0,              // (query, row) pairs that pass the predicate          -> hvs_timing.pairs
    HVS_CNT_SCANNED = 1,            // pairs a kernel evaluated or filtered                -> hvs_timing.scanned_pairs
    HVS_CNT_RESCORED = 2,           // filter survivors handed to the exact re-scoring     -> hvs_timing.rescored_pairs
    HVS_CNT_UNUSED_3 = 3,
    // base handed to the exact engine's batches whose pairs must not reach the report (re-runs of the exact list; sub-batches
    // whose pairs were counted beforehand): their PAIRS and SCANNED land in slots 4 and 5, which nothing reads
    HVS_CNT_RERUN_SINK = 4,
    HVS_CNT_RERUN_SINK_SCANNED = 5,
    HVS_CNT_UNUSED_6 = 6,
    HVS_CNT_UNUSED_7 = 7,
    HVS_CNT_DEAD_SURVIVORS = 8,     // survivors dropped because the row is dead           -> hvs_mask_info.dead_survivors
    HVS_CNT_TAIL_PAIRS = 9,         // rows behind the index: pairs evaluated              -> hvs_append_info.tail_pairs
    HVS_CNT_TAIL_KEYS = 10,         // ... keys admitted                                   -> hvs_append_info.tail_admitted
    HVS_CNT_STALE_PAIRS = 11,       // stale rows: pairs evaluated                         -> hvs_update_info.stale_pairs
    HVS_CNT_STALE_KEYS = 12,        // ... keys admitted                                   -> hvs_update_info.stale_admitted
    HVS_CNT_STALE_SURVIVORS = 13,   // survivors dropped for staleness alone               -> hvs_update_info.stale_survivors
    HVS_CNT_WITHIN_SLOTS = 14,      // distance caps: slots kept                           -> hvs_within_info.within_slots
    HVS_CNT_WITHIN_UNDERFULL = 15,  // ... queries left with fewer than k                  -> hvs_within_info.underfull_queries
    HVS_CNT_AFTER_SLOTS = 16,       // result cursors: slots kept                          -> hvs_after_info.after_slots
    HVS_CNT_AFTER_UNDERFULL = 17,   // ... queries left with fewer than k                  -> hvs_after_info.underfull_queries
    HVS_CNT_AFTER_EXHAUSTED = 18,   // ... cursors behind every key                        -> hvs_after_info.exhausted_queries
    HVS_CNT_UNUSED_19 = 19,
    HVS_CNT_EXCL_SLOTS = 20,        // exclusion lists: slots kept                         -> hvs_exclude_info.kept_slots
    HVS_CNT_EXCL_UNDERFULL = 21,    // ... queries left with fewer than k                  -> hvs_exclude_info.underfull_queries
    HVS_CNT_EXCL_REFUSED = 22,      // ... keys dropped at an admission point for being listed -> hvs_exclude_info.refused_keys
    HVS_CNT_UNUSED_23 = 23,
    // (slots 24..27 are 20..23 as seen from HVS_CNT_RERUN_SINK: an exact re-run's refused keys land in slot 26, which
    // hvs_exclude_stats adds to slot 22 -- the re-run is the pass that gave the query's answer)
    HVS_CNT_RERUN_SINK_EXCL_REFUSED = 26,
    HVS_CNT_UNUSED_27 = 27,
    HVS_CNT_CAND_SLOTS = 28,        // candidate lists: slots kept                         -> hvs_candidates_info.kept_slots
    HVS_CNT_CAND_UNDERFULL = 29,    // ... queries left with fewer than k                  -> hvs_candidates_info.underfull_queries
    HVS_CNT_SET_SLOTS = 30,         // shared row sets: slots kept                         -> hvs_row_sets_info.kept_slots
    HVS_CNT_SET_UNDERFULL = 31,     // ... queries left with fewer than k                  -> hvs_row_sets_info.underfull_queries
    HVS_CNT_SET_REFUSED = 32,       // ... keys dropped at an admission point for being outside the set -> hvs_row_sets_info.refused_keys
    HVS_CNT_SET_RESTRICTED = 33,    // ... queries answered that carry a set index         -> hvs_row_sets_info.restricted_queries
    // (slots 34..37 are 30..33 as seen from HVS_CNT_RERUN_SINK, as 24..27 are 20..23)
    HVS_CNT_RERUN_SINK_SET_REFUSED = 36,
    HVS_CNT_UNUSED_37 = 37,
    HVS_CNT_COUNT = 38
};
// the host reads these as runs (one copy each), and hvs_scan_rows_into_lists writes slots CNT and CNT + 1
static_assert(HVS_CNT_SCANNED == HVS_CNT_PAIRS + 1 && HVS_CNT_RESCORED == HVS_CNT_PAIRS + 2, "hvs_timing's three counts are one run");
static_assert(HVS_CNT_RERUN_SINK_SCANNED == HVS_CNT_RERUN_SINK + HVS_CNT_SCANNED, "the sink takes a batch's PAIRS and SCANNED");
static_assert(HVS_CNT_TAIL_KEYS == HVS_CNT_TAIL_PAIRS + 1, "hvs_scan_rows_into_lists: keys admitted follow pairs evaluated");
static_assert(HVS_CNT_STALE_KEYS == HVS_CNT_STALE_PAIRS + 1 && HVS_CNT_STALE_SURVIVORS == HVS_CNT_STALE_PAIRS + 2, "one run, and CNT + 1");
static_assert(HVS_CNT_WITHIN_UNDERFULL == HVS_CNT_WITHIN_SLOTS + 1, "hvs_within_stats reads one run");
static_assert(HVS_CNT_AFTER_UNDERFULL == HVS_CNT_AFTER_SLOTS + 1 && HVS_CNT_AFTER_EXHAUSTED == HVS_CNT_AFTER_SLOTS + 2, "hvs_after_stats reads one run");
static_assert(HVS_CNT_EXCL_UNDERFULL == HVS_CNT_EXCL_SLOTS + 1 && HVS_CNT_EXCL_REFUSED == HVS_CNT_EXCL_SLOTS + 2, "hvs_exclude_stats reads one run");
static_assert(HVS_CNT_RERUN_SINK_EXCL_REFUSED == HVS_CNT_RERUN_SINK + HVS_CNT_EXCL_REFUSED && HVS_CNT_RERUN_SINK_EXCL_REFUSED < HVS_CNT_COUNT,
              "a kernel that counts through the sink base stays inside the block");
static_assert(HVS_CNT_CAND_UNDERFULL == HVS_CNT_CAND_SLOTS + 1, "hvs_candidates_stats reads one run");
static_assert(HVS_CNT_SET_UNDERFULL == HVS_CNT_SET_SLOTS + 1 && HVS_CNT_SET_REFUSED == HVS_CNT_SET_SLOTS + 2 &&
                  HVS_CNT_SET_RESTRICTED == HVS_CNT_SET_SLOTS + 3,
              "hvs_row_sets_stats reads one run");
static_assert(HVS_CNT_RERUN_SINK_SET_REFUSED == HVS_CNT_RERUN_SINK + HVS_CNT_SET_REFUSED && HVS_CNT_RERUN_SINK_SET_REFUSED < HVS_CNT_COUNT,
              "a kernel that counts through the sink base stays inside the block");

// ---------------------------------------------------------------------------------------------
// Query parameters: reference include/optimized_parallel.hpp:93-96
//   query_type = uint32(q[0]); v = int32(q[1]) (truncation); l = q[2]; r = q[3]
// `nodes[j][0] == v` compares the row's float with float(v).  uint32(t) truncates toward zero, so t in (-1, 0) is
// type 0, and int32(-2^31) is INT_MIN (both conversions are defined).  Types outside 0..3 (and values whose
// conversion is undefined behaviour in the reference) match no row: type 4.
// ---------------------------------------------------------------------------------------------
struct HvsQParams {
    uint32_t type;
    float vf, l, r;
};

__device__ __forceinline__ HvsQParams hvs_parse_query(const float* __restrict__ q)
{
    HvsQParams p;
    const float t = q[0];
    p.type = (t > -1.0f && t < 4.0f) ? (uint32_t)(int32_t)t : 4u;
    const float v = q[1];
    if (v >= -2147483648.0f && v < 2147483648.0f) {
        p.vf = (float)(int32_t)v;
    } else {
        p.vf = 0.0f;
        if (p.type == 1u || p.type == 3u) p.type = 4u;
    }
    p.l = q[2];
    p.r = q[3];
    return p;
}

// reference include/optimized_parallel.hpp:105-138
__device__ __forceinline__ bool hvs_row_passes(const HvsQParams& p, float C, float T)
{
    const bool ceq = (C == p.vf);
    const bool tin = (T >= p.l) && (T <= p.r);
    return p.type == 0u || (p.type == 1u && ceq) || (p.type == 2u && tin) || (p.type == 3u && ceq && tin);
}

// ---------------------------------------------------------------------------------------------
// Exact-order squared L2 (reference include/optimized_impl.h:96-125 + hsum :37-47):
// 8 strided accumulators, 12 full 8-wide steps over dims 0..95, masked tail adding dims
// 96..99 into accumulators 4..7 (accumulators 0..3 add +0.0f), reduction tree
// ((a0+a4)+(a1+a5)) + ((a2+a6)+(a3+a7)).  sub, mul, add are separate f32 roundings.
// `d` and `q` are indexable by a compile-time constant (register arrays or pointers).
// ---------------------------------------------------------------------------------------------
template <typename DV, typename QV>
__device__ __forceinline__ float hvs_exact_dist(const DV& d, const QV& q)
{
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.0f;
#pragma unroll
    for (int b = 0; b < 12; ++b) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float t = d[8 * b + j] - q[8 * b + j];
            t = t * t;
            acc[j] = acc[j] + t;
        }
    }
#pragma unroll
    for (int j = 4; j < 8; ++j) {
        float t = d[92 + j] - q[92 + j];
        t = t * t;
        acc[j] = acc[j] + t;
    }
    // accumulators 0..3 add +0.0f in the reference's masked step: x + 0.0f == x for x >= +0
    const float s0 = acc[0] + acc[4];
    const float s1 = acc[1] + acc[5];
    const float s2 = acc[2] + acc[6];
    const float s3 = acc[3] + acc[7];
    const float a = s0 + s1;
    const float b2 = s2 + s3;
    return a + b2;
}

// Packed form of the same arithmetic for gfx950's v_pk_add_f32 / v_pk_mul_f32 (two f32 lanes per
// VGPR pair, each lane an independent IEEE operation, so the bits are those of the scalar form).
// acc2[k] holds accumulators (2k, 2k+1); dims (8b+2k, 8b+2k+1) feed acc2[k]; the masked tail puts
// dims 96..99 into accumulators 4..7 = acc2[2], acc2[3]; the hsum tree
// ((a0+a4)+(a1+a5)) + ((a2+a6)+(a3+a7)) starts with two packed adds.
// `d2` / `q2` are indexable sequences of 50 float pairs (dims 2i, 2i+1).
typedef float hvs_f2 __attribute__((ext_vector_type(2)));

template <typename DV2, typename QV2>
__device__ __forceinline__ float hvs_exact_dist_pk(const DV2& d2, const QV2& q2)
{
    hvs_f2 acc2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) acc2[k] = hvs_f2{0.0f, 0.0f};
#pragma unroll
    for (int b = 0; b < 12; ++b) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            hvs_f2 t = d2[4 * b + k] - q2[4 * b + k];
            t = t * t;
            acc2[k] = acc2[k] + t;
        }
    }
#pragma unroll
    for (int k = 2; k < 4; ++k) {
        hvs_f2 t = d2[46 + k] - q2[46 + k];
        t = t * t;
        acc2[k] = acc2[k] + t;
    }
    const hvs_f2 s01 = acc2[0] + acc2[2];  // (a0+a4, a1+a5)
    const hvs_f2 s23 = acc2[1] + acc2[3];  // (a2+a6, a3+a7)
    const float a = s01.x + s01.y;
    const float b2 = s23.x + s23.y;
    return a + b2;
}

// Sequential-order squared L2 of the reference's BASELINE engine (include/baseline.hpp:53-64,
// compare_with_id) and of the .dist side file (include/io.h:38-48): sum = sum + diff*diff for
// dims 0..99 in order.  A different f32 value than the SIMD order above (the reference documents
// the discrepancy, optimized.hpp:34-42 and src/fp_inaccuracy_test.cpp).
template <typename DV, typename QV>
__device__ __forceinline__ float hvs_scalar_order_dist(const DV& d, const QV& q)
{
    float sum = 0.0f;
#pragma unroll
    for (int i = 0; i < HVS_NDIM; ++i) {
        float t = d[i] - q[i];
        t = t * t;
        sum = sum + t;
    }
    return sum;
}

// ---------------------------------------------------------------------------------------------
// Candidate keys: (distance bits << 32) | row id.  Distances are sums of squares (>= +0), so
// their IEEE bit patterns order like unsigned integers and ascending u64 order is exactly the
// canonical result order (dist asc, id asc) of SURVEY.md 8c.  Non-finite distances (inf/NaN components or
// overflow) get a defined place: +inf after every finite value, NaN (one canonical bit pattern) after +inf.  The
// reference admits any row while its list is not full (optimized_impl.h:301-304: add_new_vec = not_full || better)
// and then sorts with std::sort, whose result for NaN keys is unspecified -- this order is the build's own choice there.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t hvs_make_key(float dist, uint32_t id)
{
    const uint32_t bits = (dist != dist) ? 0x7FC00000u : __float_as_uint(dist);
    return ((uint64_t)bits << 32) | (uint64_t)id;
}
__device__ __forceinline__ float hvs_key_dist(uint64_t key) { return __uint_as_float((uint32_t)(key >> 32)); }
__device__ __forceinline__ uint32_t hvs_key_id(uint64_t key) { return (uint32_t)key; }

// number of set bits of `mask` below this lane
__device__ __forceinline__ uint32_t hvs_prefix_count(uint64_t mask)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// ---------------------------------------------------------------------------------------------
// wave_select_prune: the wave-level counterpart of the reference's Knn container bookkeeping
// (include/optimized_impl.h:284-311 check_add/find_worst, :337-385 merge): instead of evicting
// the worst slot on every insertion, candidates are appended to a list and the list is cut back
// to its KEEP smallest keys when it fills up.  MSB-first radix select over the 64-bit keys
// (ballot + popcount per bit), then an in-place ordered compaction.  Keys must be distinct.
// All 64 lanes must call it (wave-uniform control flow).  `list` holds `cnt` <= 256 keys in
// memory visible to the whole wave.  Returns the KEEP-th smallest key; the list then holds
// exactly KEEP keys.  Precondition: cnt > KEEP.
// ---------------------------------------------------------------------------------------------
// Same contract, 8 bits per step instead of 1: a 256-bucket histogram of the undecided digit in wave-private LDS
// (`hist`, 256 x u32), one wave-wide prefix scan to find the bucket that holds the KEEP-th key, repeat inside that
// bucket.  Distances of one query's candidates separate within ~3 digits below their common prefix, against
// ~25 single-bit steps of 4 ballots each: the merge kernels spend 5-6x fewer instructions here.
// NK = keys per lane: the list holds at most 64 NK keys (256 for k <= 128, 512 for k <= 256); `keep` = k at run time.
// COMPACT = false: only the keep-th smallest key is returned, the list is left as it is.
template <int NK, bool COMPACT = true>
__device__ __forceinline__ uint64_t hvs_wave_select_prune(uint64_t* list, uint32_t cnt, uint32_t keep, uint32_t lane, uint32_t* hist)
{
    uint64_t k[NK];
    bool act[NK];
    bool valid[NK];
#pragma unroll
    for (int i = 0; i < NK; ++i) {
        const uint32_t idx = lane + 64u * i;
        act[i] = idx < cnt;
        valid[i] = act[i];
        k[i] = act[i] ? list[idx] : ~0ull;
    }
    // common prefix of all keys (see the bit-serial version)
    int hi;
    uint64_t prefix;
    {
        const uint64_t k0 = list[0];
        uint64_t d = 0;
#pragma unroll
        for (int i = 0; i < NK; ++i) d |= act[i] ? (k[i] ^ k0) : 0ull;
        uint32_t dlo = (uint32_t)d, dhi = (uint32_t)(d >> 32);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            dlo |= (uint32_t)__shfl_xor((int)dlo, o);
            dhi |= (uint32_t)__shfl_xor((int)dhi, o);
        }
        d = ((uint64_t)__builtin_amdgcn_readfirstlane(dhi) << 32) | __builtin_amdgcn_readfirstlane(dlo);
        hi = d ? 63 - (int)__builtin_clzll(d) : 0;
        prefix = hi < 63 ? (k0 & (~0ull << (hi + 1))) : 0ull;
    }
    uint32_t r = keep;  // rank of the wanted key inside the active set
    for (;;) {          // wave-uniform
        const int lo = hi >= 7 ? hi - 7 : 0;
        const uint32_t dmask = (1u << (hi - lo + 1)) - 1u;
#pragma unroll
        for (int i = 0; i < 4; ++i) hist[lane + 64u * i] = 0u;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
#pragma unroll
        for (int i = 0; i < NK; ++i)
            if (act[i]) atomicAdd(&hist[(uint32_t)(k[i] >> lo) & dmask], 1u);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        // lane l owns buckets 4l .. 4l+3
        const uint32_t c0 = hist[4u * lane], c1 = hist[4u * lane + 1u], c2 = hist[4u * lane + 2u], c3 = hist[4u * lane + 3u];
        const uint32_t mine = c0 + c1 + c2 + c3;
        uint32_t incl = mine;  // inclusive scan over the lanes
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, o);
            incl += lane >= (uint32_t)o ? up : 0u;
        }
        const uint32_t b0 = incl - mine, b1 = b0 + c0, b2 = b1 + c1, b3 = b2 + c2;  // keys in buckets before mine
        // exactly one bucket has  before < r <= before + count
        const bool h0 = b0 < r && r <= b0 + c0, h1 = b1 < r && r <= b1 + c1, h2 = b2 < r && r <= b2 + c2,
                   h3 = b3 < r && r <= b3 + c3;
        const uint32_t jd = h0 ? 0u : h1 ? 1u : h2 ? 2u : 3u;
        const uint32_t jb = h0 ? b0 : h1 ? b1 : h2 ? b2 : b3;
        const uint32_t jc = h0 ? c0 : h1 ? c1 : h2 ? c2 : c3;
        const uint64_t hm = __ballot(h0 | h1 | h2 | h3);
        const int src = (int)__builtin_ctzll(hm | (1ull << 63));
        const uint32_t digit = 4u * (uint32_t)src + __builtin_amdgcn_readlane(jd, src);
        const uint32_t before = __builtin_amdgcn_readlane(jb, src);
        const uint32_t rem = __builtin_amdgcn_readlane(jc, src);
        r -= before;
        prefix |= (uint64_t)digit << lo;
#pragma unroll
        for (int i = 0; i < NK; ++i) act[i] = act[i] && (((uint32_t)(k[i] >> lo) & dmask) == digit);
        if (rem == 1u) {
            // one key left under this prefix: it is the answer (keys are distinct)
#pragma unroll
            for (int i = 0; i < NK; ++i) {
                const uint64_t mm = __ballot(act[i]);
                if (mm != 0ull) {
                    const int s2 = (int)__builtin_ctzll(mm);
                    const uint32_t klo = __builtin_amdgcn_readlane((uint32_t)k[i], s2);
                    const uint32_t khi = __builtin_amdgcn_readlane((uint32_t)(k[i] >> 32), s2);
                    prefix = ((uint64_t)khi << 32) | klo;
                }
            }
            break;
        }
        if (lo == 0) break;  // every bit decided: prefix is the key
        hi = lo - 1;
    }
    if constexpr (!COMPACT) return prefix;
    uint32_t base = 0;
#pragma unroll
    for (int i = 0; i < NK; ++i) {
        const bool kp = valid[i] && k[i] <= prefix;
        const uint64_t mask = __ballot(kp);
        if (kp) list[base + hvs_prefix_count(mask)] = k[i];
        base += (uint32_t)__popcll(mask);
    }
    return prefix;
}

template <int NK>
__device__ __forceinline__ uint64_t hvs_wave_select_prune(uint64_t* list, uint32_t cnt, uint32_t keep, uint32_t lane)
{
    uint64_t k[NK];
    bool valid[NK];
#pragma unroll
    for (int i = 0; i < NK; ++i) {
        const uint32_t idx = lane + 64u * i;
        valid[i] = idx < cnt;
        k[i] = valid[i] ? list[idx] : ~0ull;
    }
    uint64_t prefix = 0;
    uint32_t r = keep;
    uint32_t rem = cnt;  // keys that still match the decided prefix bits
    // Bits above the highest bit in which any two keys differ are common to all keys (distances of one query's
    // candidates share sign, exponent and often the first mantissa bits): they go into the prefix without a
    // counting step each.
    int top = 63;
    {
        const uint64_t k0 = list[0];  // cnt > KEEP >= 1: a valid key
        uint64_t d = 0;
#pragma unroll
        for (int i = 0; i < NK; ++i) d |= valid[i] ? (k[i] ^ k0) : 0ull;
        uint32_t dlo = (uint32_t)d, dhi = (uint32_t)(d >> 32);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            dlo |= (uint32_t)__shfl_xor((int)dlo, o);
            dhi |= (uint32_t)__shfl_xor((int)dhi, o);
        }
        d = ((uint64_t)dhi << 32) | dlo;
        d = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(d >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)d);
        top = d ? 63 - (int)__builtin_clzll(d) : 0;  // (d == 0 cannot happen: keys are distinct and cnt > 1)
        prefix = top < 63 ? (k0 & (~0ull << (top + 1))) : 0ull;
    }
    for (int bit = top; bit >= 0; --bit) {
        const uint64_t himask = (bit == 63) ? 0ull : (~0ull << (bit + 1));
        uint32_t c0 = 0;
#pragma unroll
        for (int i = 0; i < NK; ++i) {
            const bool m = valid[i] && (((k[i] ^ prefix) & himask) == 0ull) && (((k[i] >> bit) & 1ull) == 0ull);
            c0 += (uint32_t)__popcll(__ballot(m));
        }
        if (r > c0) {
            r -= c0;
            rem -= c0;
            prefix |= (1ull << bit);
        } else {
            rem = c0;
        }
        if (rem == 1u) {
            // one key left under this prefix: it is the answer (keys are distinct), no need to walk
            // the remaining bits (distances usually separate within the first ~25 bits)
            const uint64_t lomask = ~0ull << bit;
#pragma unroll
            for (int i = 0; i < NK; ++i) {
                const uint64_t mm = __ballot(valid[i] && (((k[i] ^ prefix) & lomask) == 0ull));
                if (mm != 0ull) {
                    const int src = (int)__builtin_ctzll(mm);
                    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)k[i], src);
                    const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(k[i] >> 32), src);
                    prefix = ((uint64_t)hi << 32) | lo;
                }
            }
            break;
        }
    }
    uint32_t base = 0;
#pragma unroll
    for (int i = 0; i < NK; ++i) {
        const bool kp = valid[i] && k[i] <= prefix;
        const uint64_t mask = __ballot(kp);
        if (kp) list[base + hvs_prefix_count(mask)] = k[i];
        base += (uint32_t)__popcll(mask);
    }
    return prefix;
}

// ---------------------------------------------------------------------------------------------
// The tail of the merge family: one wave holds up to CAP keys (dist bits << 32 | id) of one query in its LDS buffer
// `buf`, with `hist` the 256 words of hvs_wave_select_prune.  A kernel gathers in its own way and ends with the same four steps:
// hvs_wave_final_cut, its counters, hvs_wave_pad, hvs_wave_rank_write; while it gathers, hvs_wave_make_room keeps the next
// step's slots free.  All 64 lanes call each function under wave-uniform control flow; the workgroup fences stand where the
// LDS accesses around them need them (a wave's lanes read what other lanes of the wave wrote).  The pointer parameters carry
// no __restrict__: the kernels' own qualifiers reach the inlined code, and a second set of alias scopes moved register counts.
// ---------------------------------------------------------------------------------------------
// a wave-uniform 64-bit value, moved to scalar registers
__device__ __forceinline__ uint64_t hvs_wave_uniform(uint64_t v)
{
    return ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)v);
}

// In front of a step that appends up to `step` keys: when they might not fit, the buffer is cut back to its knn smallest keys
// (knn + step <= CAP, keys distinct).  Returns the keys held; where it cut and `kth` is given, *kth is the largest key kept.
template <int CAP>
__device__ __forceinline__ uint32_t hvs_wave_make_room(uint64_t* buf, uint32_t* hist, uint32_t cnt, uint32_t step, uint32_t knn, uint32_t lane,
                                                       uint64_t* kth = nullptr)
{
    if (cnt + step > (uint32_t)CAP) {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        const uint64_t k = hvs_wave_select_prune<CAP / 64>(buf, cnt, knn, lane, hist);
        if (kth) *kth = hvs_wave_uniform(k);
        cnt = knn;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    }
    return cnt;
}

// After the gather: the knn smallest of the keys held (distinct) stay.  Returns their number, <= knn.
template <int CAP>
__device__ __forceinline__ uint32_t hvs_wave_final_cut(uint64_t* buf, uint32_t* hist, uint32_t cnt, uint32_t knn, uint32_t lane)
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    if (cnt > knn) {
        hvs_wave_select_prune<CAP / 64>(buf, cnt, knn, lane, hist);
        cnt = knn;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    }
    return cnt;
}

// The reference's padding (optimized_parallel.hpp:149-157): an answer of cnt < knn matched rows is filled up from the END of D,
// rows n - 1, n - 2, ... whatever their predicate and whether or not they are among the matched ones, with distances by the
// same exact-order function.  Slot cnt + s takes key_of(s), s = 0 .. knn - cnt - 1 -- the kernel says which row that is and
// how its distance is read --, or with pad == 0 (partial answers that are merged later) the largest key, which no row has.
template <typename KeyOf>
__device__ __forceinline__ void hvs_wave_pad(uint64_t* buf, uint32_t cnt, uint32_t knn, int pad, uint32_t lane, KeyOf key_of)
{
    for (uint32_t base = cnt; base < knn; base += 64u) {
        const uint32_t e = base + lane;
        if (e < knn) buf[e] = pad ? key_of(e - cnt) : ~0ull;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
}

// The two common pad keys of row `id` of D: against one query vector, and the smallest over the query rows [s0, s1) of Qx.
template <bool SCALAR_ORDER>
__device__ __forceinline__ uint64_t hvs_row_key(const float* D, uint32_t id, const float* qv)
{
    const float* dv = D + (size_t)id * HVS_DCOLS + 2;
    return hvs_make_key(SCALAR_ORDER ? hvs_scalar_order_dist(dv, qv) : hvs_exact_dist(dv, qv), id);
}
template <bool SCALAR_ORDER>
__device__ __forceinline__ uint64_t hvs_row_key_min(const float* D, uint32_t id, const float* Qx, uint32_t s0, uint32_t s1)
{
    uint64_t key = ~0ull;
    for (uint32_t j = s0; j < s1; ++j) {
        const uint64_t kj = hvs_row_key<SCALAR_ORDER>(D, id, Qx + (size_t)j * HVS_QCOLS + 4);
        key = kj < key ? kj : key;
    }
    return key;
}

// Rank sort of exactly knn keys in the canonical order (dist ascending, id ascending; duplicates are possible after padding:
// ties broken by slot), written to result row `row`: ids, and distances where out_dists is not null (+inf for the key ~0).
__device__ __forceinline__ void hvs_wave_rank_write(const uint64_t* buf, uint32_t knn, uint32_t lane, uint32_t row,
                                                    uint32_t* out_ids, float* out_dists)
{
    for (uint32_t e = lane; e < knn; e += 64u) {
        const uint64_t ke = buf[e];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < knn; ++j) {
            const uint64_t kj = buf[j];
            rank += (kj < ke || (kj == ke && j < e)) ? 1u : 0u;
        }
        out_ids[(size_t)row * knn + rank] = hvs_key_id(ke);
        if (out_dists) out_dists[(size_t)row * knn + rank] = ke == ~0ull ? __builtin_inff() : hvs_key_dist(ke);
    }
}
