// hvs_set_scan.h -- scanned row sets: a shared row set whose population is at most
// hvs_set_row_set_scan_limit is answered by gathering its MEMBERS by id and evaluating the exact-order distance on each, not by
// walking the index with the set's bit as one more admission test.  Seven kernels:
//   hvs_k_row_set_popcount, hvs_k_row_set_fill        the member lists, from the 32-bit set words
//   hvs_k_group_count, hvs_k_group_offsets, hvs_k_group_scatter
//                                                     a counting sort of the resident queries by set index
//   hvs_k_scan_set_members                            (set, tile of <= 256 queries, chunk of members) -> a partial list per query
//   hvs_k_merge_set_chunks                            a query's partial lists -> its result row
// None of them shares an instruction with the kernels of hvs_kernels.h / hvs_filter.h: they call the same device functions
// (hvs_row_passes, hvs_exact_dist_pk_lds, hvs_scalar_order_dist, hvs_wave_select_prune, the wave-level merge tail), so the
// distances and the key order are the other engines' to the bit.  The launchers are at the end of the file.
#pragma once

#include "hvs_kernels.h"

// One work item of hvs_k_scan_set_members (= hvs_row_set_scan_item of include/hvs.h; hvs.hip asserts it): queries
// order[q_begin .. q_end) of set `set` (at most 256) against members [m_begin, m_end) of the set's list; the query at
// order[q_begin + j] leaves its partial list in slot `slot + j`.
struct HvsScanItem {
    uint32_t set, q_begin, q_end, m_begin, m_end, slot;
};

#define HVS_SETSCAN_SPAN 2048u  // set words per block of the two member-list kernels: 8 steps of 256 threads
#define HVS_GROUP_SPAN 4096u    // queries per block (one wave) of the grouping kernels: 64 steps of 64 lanes
#define HVS_GROUP_BINS 257u     // a bin per set (HVS_ROW_SETS_MAX) and one for the queries that carry none

// the arguments of the scan and of the merge, by the names the kernels give them
struct HvsSetScanArgs {
    const float* D;
    uint32_t n, sn;
    const float* Q;
    const uint32_t* order;
    uint32_t nq;
    const HvsScanItem* items;
    const uint32_t *mem_off, *members, *live;
    const float* caps;
    const uint64_t* after_lo;
    const uint32_t *ex_begin, *ex_count, *ex_ids;  // the exclusion lists (all null: none attached)
    const uint32_t* set_of;
    uint32_t n_sets;
    const uint32_t *goff, *set_item0, *set_chunks;
    uint64_t* lists;
    uint32_t* list_cnt;
    int pad;
    const uint32_t* pad_ids;
    uint32_t* out_ids;
    float* out_dists;
    uint32_t knn;
    unsigned long long* counters;
};

static_assert(HVS_GROUP_BINS == HVS_ROW_SETS_MAX_ + 1u, "a bin per set and one more");

// word w of a set with the bits outside the window of global rows [g0, g1) cleared
__device__ __forceinline__ uint32_t hvs_set_window_word(const uint32_t* __restrict__ set, uint32_t w, uint32_t g0, uint32_t g1)
{
    uint32_t v = set[w];
    const uint64_t lo = (uint64_t)w << 5;
    if (g0 > lo) v &= g0 - lo >= 32u ? 0u : ~0u << (uint32_t)(g0 - lo);
    if (g1 < lo + 32u) v &= g1 <= lo ? 0u : (1u << (uint32_t)(g1 - lo)) - 1u;
    return v;
}
// exclusive prefix of `v` over the 256 threads of a block and their sum (`swave`: 4 words of LDS; two barriers)
__device__ __forceinline__ uint32_t hvs_block_excl_scan(uint32_t v, uint32_t* swave, uint32_t& total)
{
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, o);
        incl += lane >= (uint32_t)o ? up : 0u;
    }
    __syncthreads();  // (the words' readers of the step before are done)
    if (lane == 63u) swave[w] = incl;
    __syncthreads();
    const uint32_t s0 = swave[0], s1 = swave[1], s2 = swave[2], s3 = swave[3];
    total = s0 + s1 + s2 + s3;
    return incl - v + (w > 0u ? s0 : 0u) + (w > 1u ? s1 : 0u) + (w > 2u ? s2 : 0u);
}

// Populations.  Grid (blocks of HVS_SETSCAN_SPAN words over [w0, w1), set): blk[set * gridDim.x + block] = members of the set in
// the block's words, pop[set] += the same (zeroed by the host).  The window is this GPU's rows as global rows [g0, g1).
__global__ __launch_bounds__(256) void hvs_k_row_set_popcount(const uint32_t* __restrict__ bits, uint32_t set_words, uint32_t w0, uint32_t w1,
                                                              uint32_t g0, uint32_t g1, uint32_t* __restrict__ blk, uint32_t* __restrict__ pop)
{
    __shared__ uint32_t swave[4];
    const uint32_t s = blockIdx.y;
    const uint32_t* __restrict__ set = bits + (size_t)s * set_words;
    uint32_t c = 0;
#pragma unroll
    for (uint32_t i = 0; i < HVS_SETSCAN_SPAN / 256u; ++i) {
        const uint64_t w = (uint64_t)w0 + (uint64_t)blockIdx.x * HVS_SETSCAN_SPAN + i * 256u + threadIdx.x;
        if (w < w1) c += (uint32_t)__popc(hvs_set_window_word(set, (uint32_t)w, g0, g1));
    }
    uint32_t total;
    (void)hvs_block_excl_scan(c, swave, total);
    if (threadIdx.x == 0u) {
        blk[(size_t)s * gridDim.x + blockIdx.x] = total;
        if (total) atomicAdd(&pop[s], total);
    }
}

// Member lists.  The same grid.  A set whose mem_off is 0xFFFFFFFF is not scanned and costs its blocks one load.  A block's first
// entry is the sum of the counts of the blocks in front of it; inside the block every step of 256 words is scanned (a word per
// thread, its popcount) and a thread writes the members of its own word in ascending order: LOCAL ids, global row - g0.
// `pop` (what the count pass found) and `cap` (entries of `members`) bound every store.
__global__ __launch_bounds__(256) void hvs_k_row_set_fill(const uint32_t* __restrict__ bits, uint32_t set_words, uint32_t w0, uint32_t w1,
                                                          uint32_t g0, uint32_t g1, const uint32_t* __restrict__ blk,
                                                          const uint32_t* __restrict__ mem_off, const uint32_t* __restrict__ pop,
                                                          uint32_t* __restrict__ members, uint32_t cap)
{
    __shared__ uint32_t swave[4];
    const uint32_t s = blockIdx.y;
    const uint32_t off = mem_off[s];
    if (off == 0xFFFFFFFFu) return;  // block-uniform
    const uint32_t* __restrict__ set = bits + (size_t)s * set_words;
    const uint32_t mine = pop[s];
    uint32_t c = 0;
    for (uint32_t b = threadIdx.x; b < blockIdx.x; b += 256u) c += blk[(size_t)s * gridDim.x + b];
    uint32_t run;
    (void)hvs_block_excl_scan(c, swave, run);
    for (uint32_t i = 0; i < HVS_SETSCAN_SPAN / 256u; ++i) {
        const uint64_t w = (uint64_t)w0 + (uint64_t)blockIdx.x * HVS_SETSCAN_SPAN + i * 256u + threadIdx.x;
        uint32_t v = w < w1 ? hvs_set_window_word(set, (uint32_t)w, g0, g1) : 0u;
        uint32_t total;
        uint32_t pos = run + hvs_block_excl_scan((uint32_t)__popc(v), swave, total);
        for (; v; v &= v - 1u, ++pos) {
            const uint32_t g = ((uint32_t)w << 5) + (uint32_t)__builtin_ctz(v);
            if (pos < mine && (uint64_t)off + pos < cap) members[off + pos] = g - g0;
        }
        run += total;
    }
}

// ---------------------------------------------------------------------------------------------
// Query grouping: a stable counting sort of resident queries [q0, q0 + nq) by set index, over three launches.  A block is ONE wave
// and owns HVS_GROUP_SPAN consecutive queries; an index that names no set (0xFFFFFFFF) goes to bin n_sets.
//   count:   hist[block][bin], by LDS atomics
//   offsets: one block; thread `bin` turns its column of hist into exclusive prefixes over the blocks, then goff[0 .. n_sets + 1]
//            = first place of every bin (goff[n_sets + 1] = nq)
//   scatter: order[goff[bin] + hist[block][bin] + rank of the query among the block's queries of the bin] = the query
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t hvs_group_bin(const uint32_t* __restrict__ set_of, uint32_t q, uint32_t n_sets)
{
    const uint32_t s = set_of[q];
    return s < n_sets ? s : n_sets;
}
__global__ __launch_bounds__(64) void hvs_k_group_count(const uint32_t* __restrict__ set_of, uint32_t q0, uint32_t nq, uint32_t n_sets,
                                                        uint32_t* __restrict__ hist)
{
    __shared__ uint32_t sh[HVS_GROUP_BINS];
    const uint32_t lane = threadIdx.x;
    for (uint32_t b = lane; b <= n_sets; b += 64u) sh[b] = 0u;
    __syncthreads();
    for (uint32_t i = 0; i < HVS_GROUP_SPAN / 64u; ++i) {
        const uint64_t q = (uint64_t)blockIdx.x * HVS_GROUP_SPAN + i * 64u + lane;
        if (q < nq) atomicAdd(&sh[hvs_group_bin(set_of, q0 + (uint32_t)q, n_sets)], 1u);
    }
    __syncthreads();
    for (uint32_t b = lane; b <= n_sets; b += 64u) hist[(size_t)blockIdx.x * HVS_GROUP_BINS + b] = sh[b];
}
__global__ __launch_bounds__(512) void hvs_k_group_offsets(uint32_t* __restrict__ hist, uint32_t nblocks, uint32_t n_sets, uint32_t* __restrict__ goff)
{
    __shared__ uint32_t stot[HVS_GROUP_BINS];
    const uint32_t bin = threadIdx.x;
    if (bin <= n_sets) {
        uint32_t run = 0;
        for (uint32_t b = 0; b < nblocks; ++b) {
            const uint32_t c = hist[(size_t)b * HVS_GROUP_BINS + bin];
            hist[(size_t)b * HVS_GROUP_BINS + bin] = run;
            run += c;
        }
        stot[bin] = run;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t run = 0;
        for (uint32_t b = 0; b <= n_sets; ++b) {
            goff[b] = run;
            run += stot[b];
        }
        goff[n_sets + 1u] = run;
    }
}
__global__ __launch_bounds__(64) void hvs_k_group_scatter(const uint32_t* __restrict__ set_of, uint32_t q0, uint32_t nq, uint32_t n_sets,
                                                          const uint32_t* __restrict__ hist, const uint32_t* __restrict__ goff,
                                                          uint32_t* __restrict__ order)
{
    __shared__ uint32_t cur[HVS_GROUP_BINS];
    const uint32_t lane = threadIdx.x;
    for (uint32_t b = lane; b <= n_sets; b += 64u) cur[b] = goff[b] + hist[(size_t)blockIdx.x * HVS_GROUP_BINS + b];
    __syncthreads();
    for (uint32_t i = 0; i < HVS_GROUP_SPAN / 64u; ++i) {  // (wave-uniform)
        const uint64_t q = (uint64_t)blockIdx.x * HVS_GROUP_SPAN + i * 64u + lane;
        const bool have = q < nq;
        const uint32_t bin = have ? hvs_group_bin(set_of, q0 + (uint32_t)q, n_sets) : 0xFFFFFFFFu;
        uint64_t rem = __ballot(have);
        while (rem != 0ull) {  // one turn per distinct bin among the 64 queries
            const uint32_t lb = __builtin_amdgcn_readlane(bin, (int)__builtin_ctzll(rem));
            const uint64_t m = __ballot(bin == lb);
            const uint32_t base = cur[lb];
            if (bin == lb && base + hvs_prefix_count(m) < nq) order[base + hvs_prefix_count(m)] = q0 + (uint32_t)q;
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            if (lane == 0u) cur[lb] = base + (uint32_t)__popcll(m);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            rem &= ~m;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// hvs_k_scan_set_members -- the exact engine's row loop (hvs_k_scan_exact_lds) fed from a member list.  One workgroup per item:
// four waves, a LANE per QUERY of the tile (reached through order[]), the query's 100 floats in registers as packed pairs.
// The item's members are walked in blocks of HVS_LDS_ROWS: the whole workgroup gathers a block's rows by id into LDS once
// (26 pieces of 16 bytes per row: the 100 floats, then (C, T, id, -)), double-buffered, and every wave reads the rows back as
// broadcasts, so a gathered row serves up to 256 queries.  The dependent pair id -> row is never waited for in sequence: while
// block b is computed the rows of block b + 1 are in flight (their ids arrived during block b - 1) and so are the ids of block
// b + 2.  A member that is no row of the sampled prefix (`id < sn` fails; sn <= n, and the list's filler 0xFFFFFFFF fails it too)
// is never dereferenced.
// Per row, wave-uniform: `id < sn`, then the live bit (`live` != nullptr).  Per lane: hvs_row_passes; a row no lane of the wave
// wants costs one ballot.  Then the distance, the same operands in the same order as in every other engine.  Per key, as in
// hvs_k_scan_exact_lds: the threshold (strict, NaN until the first cut), the cap (`caps`), the cursor (`after_lo`), and the
// exclusion list last (`excl.begin`; each != nullptr while attached; excl.set_of is null: a member needs no set test).
// Keys go to the lane's own segment of CAP keys, lists[(slot + j) * CAP ..); a full segment is cut to knn by the whole wave
// (hvs_wave_select_prune), which lowers that lane's threshold.  Members ascend, so a later row at the threshold's distance
// never displaces a kept one.  At the end list_cnt[slot + j] < CAP keys are the lane's partial list.
// counters: HVS_CNT_PAIRS += member rows in the prefix, live and passing, per query; HVS_CNT_SCANNED += queries of the wave per
// row whose distance the wave evaluated; HVS_CNT_EXCL_REFUSED through hvs_count_refused.
// (two workgroups per CU: the query's 100 registers, a row's reads in flight and the id registers of the gather)
// ---------------------------------------------------------------------------------------------
template <bool SCALAR_ORDER, int CAP>
__global__ __launch_bounds__(256, 2) void hvs_k_scan_set_members(
    const float* __restrict__ D, uint32_t sn, const float* __restrict__ Q, const uint32_t* __restrict__ order,
    const HvsScanItem* __restrict__ items, const uint32_t* __restrict__ mem_off, const uint32_t* __restrict__ members,
    const uint32_t* __restrict__ live, const float* __restrict__ caps, const uint64_t* __restrict__ after_lo, HvsExcl excl,
    uint64_t* __restrict__ lists, uint32_t* __restrict__ list_cnt, uint32_t knn, unsigned long long* __restrict__ counters)
{
    __shared__ float4 srow[2][HVS_LDS_ROWS * HVS_LDS_ROW_F / 4];
    __shared__ uint32_t shist[4][256];  // digit histograms of the radix select
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    hvs_refused_begin(lane);
    const HvsScanItem it = items[blockIdx.x];
    const uint32_t pos = it.q_begin + threadIdx.x;
    const bool have_q = pos < it.q_end;
    const bool wave_active = it.q_begin + w * 64u < it.q_end;  // inactive waves still help staging and meet the barriers
    const uint32_t qi = order[have_q ? pos : it.q_end - 1u];   // (an item holds a query at least: the plan)
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
    const uint32_t* __restrict__ mem = members + mem_off[it.set];
    const uint32_t m0 = it.m_begin, m1 = it.m_end;

    // staging: piece e = (row r, part c): c < 25 -> floats 2+4c..5+4c of the row, c == 25 -> (C, T, id, 0)
    constexpr uint32_t kItems = HVS_LDS_ROWS * 26u;
    constexpr uint32_t kPer = (kItems + 255u) / 256u;
    float4 stg[kPer];
    uint32_t idn[kPer];  // the ids of this thread's pieces, one block ahead of their rows
    auto load_ids = [&](uint32_t j0) {
#pragma unroll
        for (uint32_t k = 0; k < kPer; ++k) {
            const uint32_t e = threadIdx.x + 256u * k;
            const uint32_t j = j0 + e / 26u;
            idn[k] = (e < kItems && j >= j0 && j < m1) ? mem[j] : 0xFFFFFFFFu;
        }
    };
    auto load_block = [&]() {
#pragma unroll
        for (uint32_t k = 0; k < kPer; ++k) {
            const uint32_t e = threadIdx.x + 256u * k;
            const uint32_t c = e % 26u, id = idn[k];
            float4 v = make_float4(0.f, 0.f, c < 25u ? 0.f : __uint_as_float(id), 0.f);
            if (id < sn) {
                const float* __restrict__ src = D + (size_t)id * HVS_DCOLS;
                if (c < 25u) {
                    const float2 a = *reinterpret_cast<const float2*>(src + 2 + 4 * c);
                    const float2 b = *reinterpret_cast<const float2*>(src + 4 + 4 * c);
                    v = make_float4(a.x, a.y, b.x, b.y);
                } else {
                    const float2 a = *reinterpret_cast<const float2*>(src);
                    v = make_float4(a.x, a.y, __uint_as_float(id), 0.f);
                }
            }
            stg[k] = v;
        }
    };
    auto store_block = [&](uint32_t buf) {
#pragma unroll
        for (uint32_t k = 0; k < kPer; ++k) {
            const uint32_t e = threadIdx.x + 256u * k;
            if (e < kItems) srow[buf][(e / 26u) * (HVS_LDS_ROW_F / 4) + (e % 26u)] = stg[k];
        }
    };

    uint64_t* __restrict__ mylist = lists + (size_t)(it.slot + threadIdx.x) * CAP;
    float tau = __builtin_nanf("");  // (NaN until the segment has been cut once: `!(dist >= tau)` admits every passing row)
    const float cap = caps ? caps[qi] : 0.0f;
    const uint64_t lo = after_lo ? after_lo[qi] : 0ull;
    uint32_t cnt = 0, npass = 0, nscan = 0;
    const uint32_t nhave = (uint32_t)__popcll(__ballot(have_q));

    load_ids(m0);
    load_block();
    load_ids(m0 + HVS_LDS_ROWS);
    store_block(0u);
    __syncthreads();
    uint32_t buf = 0;
    for (uint32_t j0 = m0; j0 < m1; j0 += HVS_LDS_ROWS) {
        const bool more = j0 + HVS_LDS_ROWS < m1;
        if (more) {
            load_block();                      // rows of the next block, by the ids fetched a block ago
            load_ids(j0 + 2u * HVS_LDS_ROWS);  // ids of the block after it
        }
        if (wave_active) {
            const uint32_t nrow = (m1 - j0) < HVS_LDS_ROWS ? (m1 - j0) : HVS_LDS_ROWS;
            for (uint32_t r = 0; r < nrow; ++r) {
                const float4* rowp = &srow[buf][r * (HVS_LDS_ROW_F / 4)];
                const float4 attr = rowp[25];
                const uint32_t id = __builtin_amdgcn_readfirstlane(__float_as_uint(attr.z));
                if (!(id < sn)) continue;                                   // (wave-uniform)
                if (live != nullptr && !hvs_row_live(live, id)) continue;  // (wave-uniform)
                const bool pass = hvs_row_passes(p, attr.x, attr.y);
                const uint64_t pmask = __ballot(pass);
                if (pmask == 0ull) continue;
                npass += (uint32_t)__popcll(pmask);
                nscan += nhave;
                float dist;
                if (SCALAR_ORDER) {
                    const HvsLdsRow1 d1{reinterpret_cast<const float*>(rowp)};
                    const HvsPairAsScalar q1{q2};
                    dist = hvs_scalar_order_dist(d1, q1);
                } else {
                    dist = hvs_exact_dist_pk_lds(rowp, q2);
                }
                bool admit = pass && !(dist >= tau);
                if (caps != nullptr) admit = admit && dist <= cap;
                admit = admit && hvs_make_key(dist, id) >= lo;
                if (admit && excl.begin != nullptr && hvs_refuse_listed(excl, qi, id)) admit = false;
                if (admit) {
                    mylist[cnt] = hvs_make_key(dist, id);
                    ++cnt;
                }
                uint64_t full = __ballot(cnt == (uint32_t)CAP);
                if (full != 0ull) {
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                    while (full != 0ull) {
                        const uint32_t l = (uint32_t)__builtin_ctzll(full);
                        full &= full - 1ull;
                        uint64_t* lst = lists + (size_t)(it.slot + w * 64u + l) * CAP;
                        const uint64_t kth = hvs_wave_select_prune<CAP / 64>(lst, (uint32_t)CAP, knn, lane, shist[w]);
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
    if (have_q) list_cnt[it.slot + threadIdx.x] = cnt;
    if (wave_active) hvs_count_refused(lane, counters);  // (wave-uniform)
    if (wave_active && lane == 0u) {
        if (npass) atomicAdd(&counters[HVS_CNT_PAIRS], (unsigned long long)npass);
        if (nscan) atomicAdd(&counters[HVS_CNT_SCANNED], (unsigned long long)nscan);
    }
}

// ---------------------------------------------------------------------------------------------
// hvs_k_merge_set_chunks -- one wave per query of order[0 .. nq), four per workgroup: the partial lists its tile's items left
// (one per chunk of its set's members; ids of different chunks are distinct, so nothing is de-duplicated) end as the merge family
// ends: hvs_wave_final_cut, the counters, hvs_wave_pad, hvs_wave_rank_write into result row order[pos].  A set of one chunk
// comes through here too.  The query at place `rel` of set s's group belongs to tile rel / 256 and is lane rel % 256 of its
// items, items[set_item0[s] + tile * set_chunks[s] + chunk].
// counters, as hvs_k_scan_candidates counts them: HVS_CNT_SET_SLOTS / _UNDERFULL / _RESTRICTED for every query, the slots /
// under-full pairs of caps, cursors (and exhausted cursors) and exclusion lists where those are attached.
// ---------------------------------------------------------------------------------------------
template <bool SCALAR_ORDER, int CAP>
__global__ __launch_bounds__(256) void hvs_k_merge_set_chunks(
    const float* __restrict__ D, uint32_t n, const float* __restrict__ Q, const uint32_t* __restrict__ order, uint32_t nq,
    const uint32_t* __restrict__ set_of, uint32_t n_sets, const uint32_t* __restrict__ goff, const HvsScanItem* __restrict__ items,
    const uint32_t* __restrict__ set_item0, const uint32_t* __restrict__ set_chunks, const uint64_t* __restrict__ lists,
    const uint32_t* __restrict__ list_cnt, const float* __restrict__ caps, const uint64_t* __restrict__ after_lo, int listed, int pad,
    const uint32_t* __restrict__ pad_ids, uint32_t* __restrict__ out_ids, float* __restrict__ out_dists, uint32_t knn,
    unsigned long long* __restrict__ counters)
{
    __shared__ uint64_t sbuf[4][CAP];
    __shared__ uint32_t shist[4][256];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t pos = blockIdx.x * 4u + w;
    if (pos >= nq) return;  // wave-uniform; waves never meet at a barrier
    uint64_t* buf = sbuf[w];
    const uint32_t qi = order[pos];
    const uint32_t s = set_of[qi];
    uint32_t cnt = 0;
    if (s < n_sets) {  // (wave-uniform; the host sends no other query here)
        const uint32_t rel = pos - goff[s], nch = set_chunks[s];
        const HvsScanItem* __restrict__ mine = items + set_item0[s] + (size_t)(rel >> 8) * nch;
        for (uint32_t c = 0; c < nch; ++c) {
            const uint32_t slot = mine[c].slot + (rel & 255u);
            uint32_t m = list_cnt[slot];
            if (m > (uint32_t)CAP) m = (uint32_t)CAP;
            const uint64_t* __restrict__ lst = lists + (size_t)slot * CAP;
            for (uint32_t off = 0; off < m; off += 64u) {
                cnt = hvs_wave_make_room<CAP>(buf, shist[w], cnt, 64u, knn, lane);
                const uint32_t take = (m - off) < 64u ? (m - off) : 64u;
                if (lane < take) buf[cnt + lane] = lst[off + lane];
                cnt += take;
            }
        }
    }
    cnt = hvs_wave_final_cut<CAP>(buf, shist[w], cnt, knn, lane);
    if (lane == 0u) {
        const unsigned long long under = cnt < knn ? 1ull : 0ull;
        if (cnt) atomicAdd(&counters[HVS_CNT_SET_SLOTS], (unsigned long long)cnt);
        if (under) atomicAdd(&counters[HVS_CNT_SET_UNDERFULL], under);
        atomicAdd(&counters[HVS_CNT_SET_RESTRICTED], 1ull);
        if (caps != nullptr) {
            if (cnt) atomicAdd(&counters[HVS_CNT_WITHIN_SLOTS], (unsigned long long)cnt);
            if (under) atomicAdd(&counters[HVS_CNT_WITHIN_UNDERFULL], under);
        }
        if (after_lo != nullptr) {
            if (cnt) atomicAdd(&counters[HVS_CNT_AFTER_SLOTS], (unsigned long long)cnt);
            if (under) atomicAdd(&counters[HVS_CNT_AFTER_UNDERFULL], under);
            if (after_lo[qi] == HVS_AFTER_NOTHING) atomicAdd(&counters[HVS_CNT_AFTER_EXHAUSTED], 1ull);
        }
        if (listed) {
            if (cnt) atomicAdd(&counters[HVS_CNT_EXCL_SLOTS], (unsigned long long)cnt);
            if (under) atomicAdd(&counters[HVS_CNT_EXCL_UNDERFULL], under);
        }
    }
    const float* __restrict__ qv = Q + (size_t)qi * HVS_QCOLS + 4;
    hvs_wave_pad(buf, cnt, knn, pad, lane, [=](uint32_t e) { return hvs_row_key<SCALAR_ORDER>(D, pad_ids ? pad_ids[e] : n - 1u - e, qv); });
    hvs_wave_rank_write(buf, knn, lane, qi, out_ids, out_dists);
}

// ---------------------------------------------------------------------------------------------
// launchers (host)
// ---------------------------------------------------------------------------------------------
// count, offsets, scatter: resident queries [q0, q0 + nq) sorted by set index into order[0 .. nq), goff[0 .. n_sets + 1]
static inline void hvs_launch_group_queries(hipStream_t stream, const uint32_t* set_of, uint32_t q0, uint32_t nq, uint32_t n_sets, uint32_t* hist,
                                            uint32_t* goff, uint32_t* order)
{
    const uint32_t nb = (nq + HVS_GROUP_SPAN - 1u) / HVS_GROUP_SPAN;
    hipLaunchKernelGGL(hvs_k_group_count, dim3(nb), dim3(64), 0, stream, set_of, q0, nq, n_sets, hist);
    hipLaunchKernelGGL(hvs_k_group_offsets, dim3(1), dim3(512), 0, stream, hist, nb, n_sets, goff);
    hipLaunchKernelGGL(hvs_k_group_scatter, dim3(nb), dim3(64), 0, stream, set_of, q0, nq, n_sets, hist, goff, order);
}

template <bool SCALAR_ORDER, int CAP>
static inline void hvs_launch_set_scan_as(hipStream_t stream, uint32_t n_items, const HvsSetScanArgs& a)
{
    const HvsExcl excl{a.ex_begin, a.ex_count, a.ex_ids, nullptr, nullptr, 0u, 0u};
    if (n_items)
        hipLaunchKernelGGL((hvs_k_scan_set_members<SCALAR_ORDER, CAP>), dim3(n_items), dim3(256), 0, stream, a.D, a.sn, a.Q, a.order, a.items, a.mem_off,
                           a.members, a.live, a.caps, a.after_lo, excl, a.lists, a.list_cnt, a.knn, a.counters);
    hipLaunchKernelGGL((hvs_k_merge_set_chunks<SCALAR_ORDER, CAP>), dim3((a.nq + 3u) / 4u), dim3(256), 0, stream, a.D, a.n, a.Q, a.order, a.nq, a.set_of,
                       a.n_sets, a.goff, a.items, a.set_item0, a.set_chunks, a.lists, a.list_cnt, a.caps, a.after_lo, a.ex_begin != nullptr ? 1 : 0,
                       a.pad, a.pad_ids, a.out_ids, a.out_dists, a.knn, a.counters);
}
// the scan over `n_items` items (none: every scanned set of the call is empty), then the merge; cap: 256 or 512 keys per list
static inline void hvs_launch_set_scan(hipStream_t stream, bool scalar_order, int cap, uint32_t n_items, const HvsSetScanArgs& a)
{
    if (cap == 512)
        scalar_order ? hvs_launch_set_scan_as<true, 512>(stream, n_items, a) : hvs_launch_set_scan_as<false, 512>(stream, n_items, a);
    else
        scalar_order ? hvs_launch_set_scan_as<true, 256>(stream, n_items, a) : hvs_launch_set_scan_as<false, 256>(stream, n_items, a);
}
