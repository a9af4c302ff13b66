// hvs_cand_split.h -- split candidate scans: while hvs_set_candidate_split is non-zero a call under candidate
// lists in which a normalised list is longer than the chunk is answered by ITEMS, not by queries.  A query's list is
// cut into pieces of `chunk` entries; an item is one piece, a wave scans an item.  Five kernels:
//   hvs_k_cand_split_count, hvs_k_cand_split_offsets, hvs_k_cand_split_fill
//                                   the item table, first_item[nq + 1] and the list of split queries, from the device's counts
//   hvs_k_scan_candidate_items      one wave per item: a single-piece query is finished in place, a piece of several leaves its
//                                   <= k nearest keys in its partial slot
//   hvs_k_merge_candidate_items     one wave per split query: its partial lists -> its result row
// The row step (hvs_cand_scan_piece) is the loop of hvs_k_scan_candidates over a sub-range of the list, the same tests in the same
// order and the same arithmetic on the same operands, and the ending (hvs_cand_finish) is that kernel's; both are written here a
// second time because hvs_k_scan_candidates keeps its text, so that a context that never splits runs the code object it ran
// (DESIGN 3.17a says what is duplicated).  The launchers are at the end of the file.
#pragma once

#include "hvs_set_scan.h"  // (hvs_block_excl_scan)

// One item: entries [first, first + len) of resident query q's normalised list.  slot: where a piece of several leaves its partial
// list (the item's own index), HVS_CAND_NO_SLOT for the only piece of its query, which the scanning wave finishes itself.
struct HvsCandItem {
    uint32_t q, first, len, slot;
};
#define HVS_CAND_NO_SLOT 0xFFFFFFFFu
#define HVS_CAND_SPLIT_SPAN 1024u  // queries per block of the planning kernels: 256 threads, four consecutive queries each

// the rule of hvs_candidates_split_plan (include/hvs.h): the pieces of a list of `count` entries
__host__ __device__ __forceinline__ uint32_t hvs_cand_pieces(uint32_t count, uint32_t chunk)
{
    const uint32_t p = count / chunk + (count % chunk ? 1u : 0u);
    return p ? p : 1u;
}

// ---------------------------------------------------------------------------------------------
// Item planning: an exclusive scan of pieces(q) over resident queries [q0, q0 + nq) in the shape of the query grouping of
// hvs_set_scan.h.  A block owns HVS_CAND_SPLIT_SPAN consecutive queries.
//   count:   blk[2 b] = items of block b, blk[2 b + 1] = its split queries (pieces > 1)
//   offsets: one wave; lanes 0 and 1 turn the two columns into exclusive prefixes, tot[0] = items, tot[1] = split queries
//   fill:    items[], first_item[0 .. nq], split_q[] (resident indices, ascending); `items_cap` and `split_cap` bound every store
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hvs_k_cand_split_count(const uint32_t* __restrict__ count, uint32_t q0, uint32_t nq, uint32_t chunk,
                                                              uint32_t* __restrict__ blk)
{
    __shared__ uint32_t swave[4];
    uint32_t ni = 0, ns = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
        const uint64_t i = (uint64_t)blockIdx.x * HVS_CAND_SPLIT_SPAN + 4u * threadIdx.x + j;
        if (i < nq) {
            const uint32_t p = hvs_cand_pieces(count[q0 + (uint32_t)i], chunk);
            ni += p;
            ns += p > 1u ? 1u : 0u;
        }
    }
    uint32_t ti, ts;
    (void)hvs_block_excl_scan(ni, swave, ti);
    (void)hvs_block_excl_scan(ns, swave, ts);
    if (threadIdx.x == 0u) {
        blk[2u * blockIdx.x] = ti;
        blk[2u * blockIdx.x + 1u] = ts;
    }
}
__global__ __launch_bounds__(64) void hvs_k_cand_split_offsets(uint32_t* __restrict__ blk, uint32_t nblocks, uint32_t* __restrict__ tot)
{
    const uint32_t col = threadIdx.x;
    if (col >= 2u) return;
    uint32_t run = 0;
    for (uint32_t b = 0; b < nblocks; ++b) {
        const uint32_t c = blk[2u * b + col];
        blk[2u * b + col] = run;
        run += c;
    }
    tot[col] = run;
}
__global__ __launch_bounds__(256) void hvs_k_cand_split_fill(const uint32_t* __restrict__ count, uint32_t q0, uint32_t nq, uint32_t chunk,
                                                             const uint32_t* __restrict__ blk, HvsCandItem* __restrict__ items, uint32_t items_cap,
                                                             uint32_t* __restrict__ first_item, uint32_t* __restrict__ split_q, uint32_t split_cap)
{
    __shared__ uint32_t swave[4];
    uint32_t len[4], ni = 0, ns = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
        const uint64_t i = (uint64_t)blockIdx.x * HVS_CAND_SPLIT_SPAN + 4u * threadIdx.x + j;
        len[j] = i < nq ? count[q0 + (uint32_t)i] : 0u;
        if (i < nq) {
            const uint32_t p = hvs_cand_pieces(len[j], chunk);
            ni += p;
            ns += p > 1u ? 1u : 0u;
        }
    }
    uint32_t total;
    uint32_t it = blk[2u * blockIdx.x] + hvs_block_excl_scan(ni, swave, total);
    uint32_t sp = blk[2u * blockIdx.x + 1u] + hvs_block_excl_scan(ns, swave, total);
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
        const uint64_t i = (uint64_t)blockIdx.x * HVS_CAND_SPLIT_SPAN + 4u * threadIdx.x + j;
        if (i >= nq) break;
        const uint32_t p = hvs_cand_pieces(len[j], chunk);
        first_item[i] = it;
        if (p > 1u) {
            if (sp < split_cap) split_q[sp] = q0 + (uint32_t)i;
            ++sp;
        }
        for (uint32_t c = 0; c < p; ++c, ++it) {
            const uint32_t first = c * chunk, rest = len[j] - first;  // (first < len[j] for c >= 1: the rule; an empty list has one empty piece)
            if (it < items_cap) items[it] = HvsCandItem{q0 + (uint32_t)i, first, rest < chunk ? rest : chunk, p > 1u ? it : HVS_CAND_NO_SLOT};
        }
        if (i + 1u == nq) first_item[nq] = it;
    }
}

// ---------------------------------------------------------------------------------------------
// The row loop of hvs_k_scan_candidates over `len` entries at `lst` (ids of a normalised list: ascending, distinct), for the wave
// that holds query q's keys in `buf`.  ROWS ids per step: 16 in SIMD order (four lanes per row), 64 in scalar order; the ids of
// the step after the next and C, T of the next are in flight while a step computes.  Per row `id < sn`, the live bit, the
// predicate; per key the cap, the cursor, tau (this wave's own: set by a cut of this piece's keys), the exclusion list.  No row
// set: a call with set indices attached is never split, `excl` carries none.  Returns the keys held; npass += rows
// that reached the distance's step as passing.
// ---------------------------------------------------------------------------------------------
template <bool SCALAR_ORDER, int CAP>
__device__ __forceinline__ uint32_t hvs_cand_scan_piece(const float* __restrict__ D, uint32_t sn, const float* __restrict__ Q, uint32_t q,
                                                        const uint32_t* __restrict__ lst, uint32_t len, const uint32_t* __restrict__ live,
                                                        const float* __restrict__ caps, const uint64_t* __restrict__ after_lo, const HvsExcl& excl,
                                                        uint64_t* buf, uint32_t* hist, uint32_t knn, uint32_t lane, uint32_t& npass)
{
    constexpr uint32_t ROWS = SCALAR_ORDER ? 64u : 16u;  // rows per step
    constexpr uint32_t LPR = 64u / ROWS;                 // lanes per row
    const HvsQParams p = hvs_parse_query(Q + (size_t)q * HVS_QCOLS);
    const float* __restrict__ qv = Q + (size_t)q * HVS_QCOLS + 4;
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
    uint32_t cnt = 0;
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
        cnt = hvs_wave_make_room<CAP>(buf, hist, cnt, ROWS, knn, lane, &tau);  // (a cut sets tau; knn + 64 <= CAP)
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
        }
        const uint64_t m = __ballot(admit);
        if (admit) buf[cnt + hvs_prefix_count(m)] = key;
        cnt += (uint32_t)__popcll(m);
    }
    return cnt;
}

// The end of a query under candidate lists, as hvs_k_scan_candidates ends it: the wave holds cnt gathered keys of query q.  The
// final cut, the per-query counters (slots and under-full counts of candidates, caps, cursors and lists, each once), the
// padding, the rank sort into result row q.
template <bool SCALAR_ORDER, int CAP>
__device__ __forceinline__ void hvs_cand_finish(const float* __restrict__ D, uint32_t n, const float* __restrict__ Q, uint32_t q, uint64_t* buf,
                                                uint32_t* hist, uint32_t cnt, const float* __restrict__ caps, const uint64_t* __restrict__ after_lo,
                                                const HvsExcl& excl, int pad, const uint32_t* __restrict__ pad_ids, uint32_t* __restrict__ out_ids,
                                                float* __restrict__ out_dists, uint32_t knn, uint32_t lane, unsigned long long* __restrict__ counters)
{
    cnt = hvs_wave_final_cut<CAP>(buf, hist, cnt, knn, lane);
    if (lane == 0u) {
        const unsigned long long under = cnt < knn ? 1ull : 0ull;
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
    const float* __restrict__ qv = Q + (size_t)q * HVS_QCOLS + 4;
    // fewer than knn admitted rows (s < knn <= live rows: host)
    hvs_wave_pad(buf, cnt, knn, pad, lane, [=](uint32_t s) { return hvs_row_key<SCALAR_ORDER>(D, pad_ids ? pad_ids[s] : n - 1u - s, qv); });
    hvs_wave_rank_write(buf, knn, lane, q, out_ids, out_dists);
}

// ---------------------------------------------------------------------------------------------
// hvs_k_scan_candidate_items -- one wave per item, four per workgroup, consecutive items in one workgroup: the pieces of one query
// run side by side and read the query row and the exclusion list from the same cache lines.  The item's fields are wave-uniform
// and live in scalar registers.  Two endings (wave-uniform):
//   the only piece of its query: hvs_cand_finish, as hvs_k_scan_candidates ends -- a short list costs what it cost there;
//   a piece of several: hvs_wave_final_cut to <= knn keys, written unpadded to partial[slot * knn ..) with partial_cnt[slot].
// counters of every item: HVS_CNT_PAIRS += passing rows, HVS_CNT_SCANNED += entries of the piece; everything counted once per query is hvs_cand_finish's, here or in the merge.
// ---------------------------------------------------------------------------------------------
template <bool SCALAR_ORDER, int CAP>
__global__ __launch_bounds__(256) void hvs_k_scan_candidate_items(const float* __restrict__ D, uint32_t n, uint32_t sn, const float* __restrict__ Q,
                                                                  const HvsCandItem* __restrict__ items, uint32_t n_items, HvsExcl cand,
                                                                  const uint32_t* __restrict__ live, const float* __restrict__ caps,
                                                                  const uint64_t* __restrict__ after_lo, HvsExcl excl, int pad,
                                                                  const uint32_t* __restrict__ pad_ids, uint32_t* __restrict__ out_ids,
                                                                  float* __restrict__ out_dists, uint32_t knn, uint64_t* __restrict__ partial,
                                                                  uint32_t* __restrict__ partial_cnt, unsigned long long* __restrict__ counters)
{
    __shared__ uint64_t sbuf[4][CAP];
    __shared__ uint32_t shist[4][256];  // digit histograms of the radix select
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = threadIdx.x >> 6;
    const uint32_t i = blockIdx.x * 4u + w;
    if (i >= n_items) return;  // wave-uniform (the last workgroup's idle waves); waves never meet at a barrier
    const uint32_t q = __builtin_amdgcn_readfirstlane(items[i].q), first = __builtin_amdgcn_readfirstlane(items[i].first);
    const uint32_t len = __builtin_amdgcn_readfirstlane(items[i].len), slot = __builtin_amdgcn_readfirstlane(items[i].slot);
    uint64_t* buf = sbuf[w];
    uint32_t npass = 0;
    uint32_t cnt = hvs_cand_scan_piece<SCALAR_ORDER, CAP>(D, sn, Q, q, cand.ids + cand.begin[q] + first, len, live, caps, after_lo, excl, buf, shist[w],
                                                          knn, lane, npass);
    if (lane == 0u) {
        if (npass) atomicAdd(&counters[HVS_CNT_PAIRS], (unsigned long long)npass);
        if (len) atomicAdd(&counters[HVS_CNT_SCANNED], (unsigned long long)len);
    }
    if (slot == HVS_CAND_NO_SLOT) {
        hvs_cand_finish<SCALAR_ORDER, CAP>(D, n, Q, q, buf, shist[w], cnt, caps, after_lo, excl, pad, pad_ids, out_ids, out_dists, knn, lane, counters);
        return;
    }
    cnt = hvs_wave_final_cut<CAP>(buf, shist[w], cnt, knn, lane);
    uint64_t* __restrict__ mine = partial + (size_t)slot * knn;
    for (uint32_t e = lane; e < cnt; e += 64u) mine[e] = buf[e];
    if (lane == 0u) partial_cnt[slot] = cnt;
}

// ---------------------------------------------------------------------------------------------
// hvs_k_merge_candidate_items -- one wave per split query, four per workgroup.  Query split_q[j] owns items first_item[q - q0] ..
// first_item[q - q0 + 1) (at most 128: 8192 entries in chunks of 64 at least), each with <= knn keys in its partial slot.  They
// are streamed through the wave's buffer 64 keys at a time: hvs_wave_make_room cuts to knn when the next step might not fit and
// hands back tau, and a key that is not below tau is not stored.  The pieces are disjoint ranges of a de-duplicated list, so the
// keys are distinct and nothing is de-duplicated.  Then hvs_cand_finish.
// ---------------------------------------------------------------------------------------------
template <bool SCALAR_ORDER, int CAP>
__global__ __launch_bounds__(256) void hvs_k_merge_candidate_items(const float* __restrict__ D, uint32_t n, const float* __restrict__ Q, uint32_t q0,
                                                                   const uint32_t* __restrict__ split_q, uint32_t n_split,
                                                                   const uint32_t* __restrict__ first_item, uint32_t n_items,
                                                                   const uint64_t* __restrict__ partial, const uint32_t* __restrict__ partial_cnt,
                                                                   const float* __restrict__ caps, const uint64_t* __restrict__ after_lo, HvsExcl excl,
                                                                   int pad, const uint32_t* __restrict__ pad_ids, uint32_t* __restrict__ out_ids,
                                                                   float* __restrict__ out_dists, uint32_t knn, unsigned long long* __restrict__ counters)
{
    __shared__ uint64_t sbuf[4][CAP];
    __shared__ uint32_t shist[4][256];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t j = blockIdx.x * 4u + w;
    if (j >= n_split) return;  // wave-uniform; waves never meet at a barrier
    uint64_t* buf = sbuf[w];
    const uint32_t q = __builtin_amdgcn_readfirstlane(split_q[j]);
    const uint32_t i0 = __builtin_amdgcn_readfirstlane(first_item[q - q0]);
    uint32_t i1 = __builtin_amdgcn_readfirstlane(first_item[q - q0 + 1u]);
    if (i1 > n_items) i1 = n_items;  // (the plan's own figures; never trusted as an address)
    uint64_t tau = ~0ull;
    uint32_t cnt = 0;
    for (uint32_t i = i0; i < i1; ++i) {
        uint32_t m = partial_cnt[i];
        if (m > knn) m = knn;
        const uint64_t* __restrict__ lst = partial + (size_t)i * knn;
        for (uint32_t off = 0; off < m; off += 64u) {
            cnt = hvs_wave_make_room<CAP>(buf, shist[w], cnt, 64u, knn, lane, &tau);
            const uint64_t key = off + lane < m ? lst[off + lane] : ~0ull;
            const bool in = key < tau;  // (no row has the key ~0)
            const uint64_t mk = __ballot(in);
            if (in) buf[cnt + hvs_prefix_count(mk)] = key;
            cnt += (uint32_t)__popcll(mk);
        }
    }
    hvs_cand_finish<SCALAR_ORDER, CAP>(D, n, Q, q, buf, shist[w], cnt, caps, after_lo, excl, pad, pad_ids, out_ids, out_dists, knn, lane, counters);
}

// ---------------------------------------------------------------------------------------------
// launchers (host)
// ---------------------------------------------------------------------------------------------
// the arguments of the scan over items and of the merge, by the names the kernels give them
struct HvsCandSplitArgs {
    const float* D;
    uint32_t n, sn;
    const float* Q;
    uint32_t q0;
    const HvsCandItem* items;
    uint32_t n_items;
    const uint32_t* split_q;
    uint32_t n_split;
    const uint32_t* first_item;
    HvsExcl cand;
    const uint32_t* live;
    const float* caps;
    const uint64_t* after_lo;
    HvsExcl excl;
    int pad;
    const uint32_t* pad_ids;
    uint32_t* out_ids;
    float* out_dists;
    uint32_t knn;
    uint64_t* partial;
    uint32_t* partial_cnt;
    unsigned long long* counters;
};

static inline uint32_t hvs_cand_split_blocks(uint32_t nq) { return (nq + HVS_CAND_SPLIT_SPAN - 1u) / HVS_CAND_SPLIT_SPAN; }

// count and offsets: blk[2 x blocks] holds the blocks' exclusive prefixes, tot[0 .. 2) the items and the split queries
static inline void hvs_launch_cand_split_count(hipStream_t stream, const uint32_t* count, uint32_t q0, uint32_t nq, uint32_t chunk, uint32_t* blk,
                                               uint32_t* tot)
{
    const uint32_t nb = hvs_cand_split_blocks(nq);
    hipLaunchKernelGGL(hvs_k_cand_split_count, dim3(nb), dim3(256), 0, stream, count, q0, nq, chunk, blk);
    hipLaunchKernelGGL(hvs_k_cand_split_offsets, dim3(1), dim3(64), 0, stream, blk, nb, tot);
}
static inline void hvs_launch_cand_split_fill(hipStream_t stream, const uint32_t* count, uint32_t q0, uint32_t nq, uint32_t chunk, const uint32_t* blk,
                                              HvsCandItem* items, uint32_t items_cap, uint32_t* first_item, uint32_t* split_q, uint32_t split_cap)
{
    hipLaunchKernelGGL(hvs_k_cand_split_fill, dim3(hvs_cand_split_blocks(nq)), dim3(256), 0, stream, count, q0, nq, chunk, blk, items, items_cap,
                       first_item, split_q, split_cap);
}

template <bool SCALAR_ORDER, int CAP>
static inline void hvs_launch_cand_split_as(hipStream_t stream, const HvsCandSplitArgs& a)
{
    hipLaunchKernelGGL((hvs_k_scan_candidate_items<SCALAR_ORDER, CAP>), dim3((a.n_items + 3u) / 4u), dim3(256), 0, stream, a.D, a.n, a.sn, a.Q, a.items,
                       a.n_items, a.cand, a.live, a.caps, a.after_lo, a.excl, a.pad, a.pad_ids, a.out_ids, a.out_dists, a.knn, a.partial, a.partial_cnt,
                       a.counters);
    if (a.n_split)
        hipLaunchKernelGGL((hvs_k_merge_candidate_items<SCALAR_ORDER, CAP>), dim3((a.n_split + 3u) / 4u), dim3(256), 0, stream, a.D, a.n, a.Q, a.q0,
                           a.split_q, a.n_split, a.first_item, a.n_items, a.partial, a.partial_cnt, a.caps, a.after_lo, a.excl, a.pad, a.pad_ids,
                           a.out_ids, a.out_dists, a.knn, a.counters);
}
// the scan over the items (one at least: a call of nq >= 1 queries), then the merge of the split queries; cap: 256 or 512 keys
static inline void hvs_launch_cand_split(hipStream_t stream, bool scalar_order, int cap, const HvsCandSplitArgs& a)
{
    if (cap == 512)
        scalar_order ? hvs_launch_cand_split_as<true, 512>(stream, a) : hvs_launch_cand_split_as<false, 512>(stream, a);
    else
        scalar_order ? hvs_launch_cand_split_as<true, 256>(stream, a) : hvs_launch_cand_split_as<false, 256>(stream, a);
}
