// hvs_tail_f16.h -- the rows behind the index (tail and stale rows) with an FP16 MFMA bound in front of the
// exact distance.  hvs_k_scan_behind_f16 is hvs_scan_rows_into_lists (hvs_filter.h) for launches that hand out
// lists under thresholds, with the staged f32 rows replaced by OPERAND BLOCKS that hvs_k_build_behind_operands prepares once per
// call: per 32 rows the half-precision A fragments of v_mfma_f32_32x32x16_f16, the rows' (A_d, e_d) terms, ids and (C, T).  A
// matrix product of a block and the wave's 64 queries gives every pair the lower bound of hvs_set_scan_f16.h -- the same
// functions, constants and proof -- against the lane's threshold, and only a pair the bound does not prove beyond it is
// evaluated: by the exact-order forms of hvs_device.h on the row in D, rows ascending per lane, through the admission sequence
// of hvs_scan_rows_into_lists.  A pair that is skipped has dist > tau for a tau no lower than the lane's at that row, so the
// unfiltered kernel refuses it without any effect on the lane: keys, cuts, thresholds, failure flags and counters are that
// kernel's, and the lists match word for word.  Chosen by hvs_set_tail_filter(ctx, 1); off by default.
//
// Measured (profiles/tail_filter_rate.txt; D = 10^7, 262 144 mixed queries, one MI355X, one run): against the unfiltered scans
// +3.4 % queries/s at 2441 tail rows, +11.9 % at 9765, +47.7 % at 39 060, +6.2 % at 9765 stale rows; no size measured at which
// it loses, so no crossover is on record.  The default stays 0.
#pragma once

#include "hvs_filter.h"
#include "hvs_set_scan_f16.h"

// One operand block, HVS_BEHIND_BLOCK_U4 uint4 = 8 KiB = eight LDS-DMA chunks of 64 x 16 bytes:
//   chunks 0..6  k-step ks: lane l holds row l & 31, components 16 ks + 8 (l >> 5) + 0..7 as halves (K = 100, zeros up to 112)
//   chunk 7      float2 (A_d, e_d)[32] | uint32 id[32] | float2 (C, T)[32] | zeros
// A short last block is filled with rows of id 0xFFFFFFFF, zero halves and NaN attributes, which no query wants.
#define HVS_BEHIND_BLOCK_U4 512u
#define HVS_BEHIND_TERMS_U4 448u  // (A_d, e_d): 16 uint4
#define HVS_BEHIND_IDS_U4 464u    // ids: 8 uint4
#define HVS_BEHIND_ATTR_U4 472u   // (C, T): 16 uint4; 488..511 zeros

// Operand blocks of the rows ids [tail_lo, tail_lo + tail_n) -- blocks [0, ceil(tail_n / 32)) -- and, behind them, of the rows
// stale_ids[0 .. stale_n).  One workgroup per block.  An id at or past n (no row of D) is treated as padding.
__global__ __launch_bounds__(256) void hvs_k_build_behind_operands(const float* __restrict__ D, uint32_t n, uint32_t tail_lo, uint32_t tail_n,
                                                                   const uint32_t* __restrict__ stale_ids, uint32_t stale_n,
                                                                   uint4* __restrict__ ops)
{
    constexpr uint32_t RB = HVS_SCANF_ROWS;
    __shared__ float2 spart[RB * 25u];  // (e^2, n^2) of every piece of 4 floats
    const uint32_t tail_blocks = (tail_n + RB - 1u) / RB;
    const bool stale = blockIdx.x >= tail_blocks;
    const uint32_t j0 = (stale ? blockIdx.x - tail_blocks : blockIdx.x) * RB;
    const uint32_t nrows = stale ? stale_n : tail_n;
    uint4* __restrict__ blk = ops + (size_t)blockIdx.x * HVS_BEHIND_BLOCK_U4;
    uint2* __restrict__ half2 = reinterpret_cast<uint2*>(blk);
    auto half_slot = [](uint32_t r, uint32_t c) { return ((c >> 2) * 64u + ((c >> 1) & 1u) * 32u + r) * 2u + (c & 1u); };
    // piece e = (row r, part c): c < 25 -> floats 2+4c..5+4c of the row, c == 25 -> (C, T), the id and the zeros of k = 100..111
    for (uint32_t e = threadIdx.x; e < RB * 26u; e += 256u) {
        const uint32_t r = e / 26u, c = e % 26u;
        uint32_t id = 0xFFFFFFFFu;
        if (j0 + r < nrows) id = stale ? stale_ids[j0 + r] : tail_lo + j0 + r;
        if (!(id < n)) id = 0xFFFFFFFFu;
        const float* __restrict__ src = D + (size_t)(id < n ? id : 0u) * HVS_DCOLS;
        if (c < 25u) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (id < n) {
                const float2 a = *reinterpret_cast<const float2*>(src + 2 + 4 * c);
                const float2 b = *reinterpret_cast<const float2*>(src + 4 + 4 * c);
                v = make_float4(a.x, a.y, b.x, b.y);
            }
            hvs_f2 h01, h23;
            spart[r * 25u + c] = hvs_scanf_part(v, h01, h23);
            half2[half_slot(r, c)] = make_uint2(hvs_scanf_pack(h01), hvs_scanf_pack(h23));
        } else {
            half2[half_slot(r, 25u)] = make_uint2(0u, 0u);
            half2[half_slot(r, 26u)] = make_uint2(0u, 0u);
            half2[half_slot(r, 27u)] = make_uint2(0u, 0u);
            float2 attr = make_float2(__builtin_nanf(""), __builtin_nanf(""));
            if (id < n) attr = *reinterpret_cast<const float2*>(src);
            reinterpret_cast<float2*>(blk + HVS_BEHIND_ATTR_U4)[r] = attr;
            reinterpret_cast<uint32_t*>(blk + HVS_BEHIND_IDS_U4)[r] = id;
        }
    }
    if (threadIdx.x < HVS_BEHIND_BLOCK_U4 - (HVS_BEHIND_ATTR_U4 + 16u)) blk[HVS_BEHIND_ATTR_U4 + 16u + threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    // per-row terms as hvs_k_scan_set_members_f16 sums them: lane l takes row l & 31, pieces 13 (l >> 5) .., in order
    if (threadIdx.x < 64u) {
        const uint32_t lane = threadIdx.x, r = lane & 31u, c0 = 13u * (lane >> 5), c1 = c0 ? 25u : 13u;
        float e2 = 0.0f, n2 = 0.0f;
        for (uint32_t c = c0; c < c1; ++c) {
            const float2 s = spart[r * 25u + c];
            e2 += s.x;
            n2 += s.y;
        }
        e2 += __shfl_xor(e2, 32);
        n2 += __shfl_xor(n2, 32);
        const float2 t = hvs_scanf_terms(e2, n2, 0.0f);
        if (lane < 32u) reinterpret_cast<float2*>(blk + HVS_BEHIND_TERMS_U4)[r] = make_float2(t.x, t.y * HVS_SCANF_TINY);
    }
}

// The filtered scan of rows [0, nrows) of the operand blocks at `ops` (the tail's blocks, or the stale rows' blocks), for the
// batch in slot layout B into the lists of O.  nrows selects a prefix: the tail rows below sn, the stale ids below sn.  One lane
// per slot, four waves per workgroup, as hvs_scan_rows_into_lists; CNT as there.  O.lists and O.tau are not null.
// Budget: two workgroups per CU (256 registers a lane: 56 of the query fragments, 32 accumulators, no f32 query), LDS 16 KiB
// of two operand blocks; no scratch.
template <bool SCALAR_ORDER, int CAP, bool MASKED, int CNT, bool AFTER, bool EXCL>
__global__ __launch_bounds__(256, 2) void hvs_k_scan_behind_f16(const float* __restrict__ D, const float* __restrict__ Q, const HvsBatch B,
                                                                const HvsTailOut O, const uint4* __restrict__ ops, uint32_t nrows,
                                                                unsigned long long* __restrict__ counters, int count,
                                                                const uint32_t* __restrict__ live, const uint64_t* __restrict__ after_lo,
                                                                HvsExcl excl)
{
    static_assert(!EXCL || AFTER, "the list forms exist on the cursor forms only");
    constexpr uint32_t RB = HVS_SCANF_ROWS, KS = HVS_SCANF_KSTEPS;
    __shared__ __attribute__((aligned(16))) uint4 sblk[2][HVS_BEHIND_BLOCK_U4];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    if constexpr (EXCL) hvs_refused_begin(lane);
    const uint32_t w = blockIdx.x * 4u + wv;
    const uint32_t slot = w * 64u + lane;
    const bool wave_active = w * 64u < B.nslots;  // inactive waves still help staging and meet the barriers
    const uint32_t knn = B.knn;

    const uint32_t qi = slot < B.nslots ? B.qid[slot] : 0xFFFFFFFFu;
    const bool have_q = qi != 0xFFFFFFFFu;
    const uint32_t qrd = have_q ? qi : 0u;
    const float* __restrict__ qrow = Q + (size_t)qrd * HVS_QCOLS;
    HvsQParams p = hvs_parse_query(qrow);
    if (!have_q) p.type = 4u;
    // the lane's own query: A_q, e_q in the fixed order of the components (nothing of it stays in registers)
    float aq, eq;
    {
        float e2 = 0.0f, n2 = 0.0f;
#pragma unroll 5
        for (int i = 0; i < HVS_NDIM / 4; ++i) {
            hvs_f2 h01, h23;
            const float2 s = hvs_scanf_part(*reinterpret_cast<const float4*>(qrow + 4 + 4 * i), h01, h23);
            e2 += s.x;
            n2 += s.y;
        }
        const float2 t = hvs_scanf_terms(e2, n2, 8e-7f);
        aq = t.x;
        eq = t.y;
    }
    // the B operand, in registers: set qb holds queries 32 qb .. 32 qb + 31 of the wave; lane l of k-step ks carries query column
    // l & 31, k = 16 ks + 8 (l >> 5) + 0..7 (the scheme of hvs_k_scan_set_members_f16), built once per launch
    hvs_f16x8 bq[2][KS];
    float aq_of[2];
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
        const int src = qb * 32 + (int)(lane & 31u);
        const uint32_t qo = (uint32_t)__shfl((int)qrd, src);
        aq_of[qb] = __shfl(aq, src);
        const float* __restrict__ orow = Q + (size_t)qo * HVS_QCOLS + 4;
#pragma unroll
        for (uint32_t ks = 0; ks < KS; ++ks) {
            const uint32_t k0 = 16u * ks + 8u * (lane >> 5);
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 lo4 = k0 + 4u <= (uint32_t)HVS_NDIM ? *reinterpret_cast<const float4*>(orow + k0) : z;
            const float4 hi4 = k0 + 8u <= (uint32_t)HVS_NDIM ? *reinterpret_cast<const float4*>(orow + k0 + 4u) : z;
            bq[qb][ks] = hvs_f16x8{(_Float16)lo4.x, (_Float16)lo4.y, (_Float16)lo4.z, (_Float16)lo4.w,
                                   (_Float16)hi4.x, (_Float16)hi4.y, (_Float16)hi4.z, (_Float16)hi4.w};
        }
    }
    // this lane's segment: places [s0, s0 + segcap) of its slot's list
    bool takes = have_q && slot >= O.slot_lo && slot < O.slot_hi;
    uint32_t s0 = takes ? O.counts[slot] : 0u;
    if (s0 > O.stride) takes = false;  // (overflowed at the last level and flagged there: the list is not used)
    if (!takes) s0 = 0u;
    const bool owns = takes;  // this lane writes its list's new fill at the end
    const uint32_t room = takes ? O.stride - s0 : 0u;
    const uint32_t segcap = room < (uint32_t)CAP ? room : (uint32_t)CAP;  // (0: a full list -- flagged only if a key needs a place)
    uint64_t* __restrict__ myseg = O.lists + (size_t)(takes ? slot : 0u) * O.stride + s0;
    float tau = takes ? O.tau[slot] : __builtin_inff();
    uint64_t key_lo = 0ull;
    if constexpr (AFTER) key_lo = have_q ? after_lo[qi] : HVS_AFTER_NOTHING;
    const float g2 = 1.0f + 2.0f * (SCALAR_ORDER ? 104.0f : 20.0f) * 5.9604644775390625e-08f;  // 1 + 2 g (sequential order: 104 roundings)
    uint32_t cnt = 0, npass = 0, nadm = 0, nrows_seen = 0, nbound = 0, nexact = 0;

    if (nrows == 0u) return;  // uniform over the grid
    const uint32_t nblk = (nrows + RB - 1u) / RB;
    // staging: a block is eight LDS-DMA chunks, two per wave; the next block is in flight under this block's products
    auto stage = [&](uint32_t b, uint32_t buf) {
        const uint4* __restrict__ src = ops + (size_t)b * HVS_BEHIND_BLOCK_U4;
#pragma unroll
        for (uint32_t h = 0; h < 2u; ++h) {
            const uint32_t chunk = wv * 2u + h;
            hvs_lds_dma(src + chunk * 64u + lane, &sblk[buf][chunk * 64u]);
        }
    };
    stage(0u, 0u);
    hvs_stage_barrier();
    uint32_t buf = 0;
    for (uint32_t b = 0; b < nblk; ++b) {
        if (b + 1u < nblk) stage(b + 1u, buf ^ 1u);
        if (wave_active) {
            const uint32_t nrow = (nrows - b * RB) < RB ? (nrows - b * RB) : RB;
            const uint32_t* __restrict__ bid = reinterpret_cast<const uint32_t*>(&sblk[buf][HVS_BEHIND_IDS_U4]);
            const float2* __restrict__ battr = reinterpret_cast<const float2*>(&sblk[buf][HVS_BEHIND_ATTR_U4]);
            // which rows count (wave-uniform: in the prefix, live) and which of them this lane's query wants
            uint32_t valid = 0, want = 0;
            for (uint32_t r = 0; r < nrow; ++r) {
                if constexpr (MASKED) {
                    const uint32_t id = __builtin_amdgcn_readfirstlane(bid[r]);
                    if (!hvs_row_live(live, id)) continue;  // (wave-uniform)
                }
                valid |= 1u << r;
                const float2 attr = battr[r];
                want |= hvs_row_passes(p, attr.x, attr.y) ? 1u << r : 0u;
            }
            nrows_seen += (uint32_t)__popc(valid);
            npass += (uint32_t)__popc(want);
            if (!takes) want = 0u;  // (the full-scan classes of the range scan: the row is counted, its distance is nobody's business)
            // the lane's threshold as X = (e_q + sqrt((tau + 1e-30)(1 + 2g))) rounded up; NaN or +inf: nothing is refused
            const float x = (eq + sqrtf((tau + 1e-30f) * g2 * HVS_SCANF_TINY) * HVS_SCANF_TINY) * HVS_SCANF_TINY;
            uint32_t need = want;
            if (__ballot(want != 0u && x < __builtin_inff()) != 0ull) {  // (wave-uniform) some lane can refuse something
                nbound += (uint32_t)__popc(valid);
                hvs_f32x16 acc[2];
#pragma unroll
                for (int qb = 0; qb < 2; ++qb)
#pragma unroll
                    for (int v = 0; v < 16; ++v) acc[qb][v] = 0.0f;
#pragma unroll
                for (uint32_t ks = 0; ks < KS; ++ks) {
                    const hvs_f16x8 a = HvsFmt<HVS_FMT_F16>::frag(sblk[buf][ks * 64u + lane]);
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bq[0][ks], acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bq[1][ks], acc[1], 0, 0, 0);
                }
                // accumulator v of a lane is row (v & 3) + 8 (v >> 2) + 4 (l >> 5) of query column l & 31 of its set
                const float4* __restrict__ bterm = reinterpret_cast<const float4*>(&sblk[buf][HVS_BEHIND_TERMS_U4]);
                uint32_t rej[2];
#pragma unroll
                for (int qb = 0; qb < 2; ++qb) {
                    const float xo = __shfl(x, qb * 32 + (int)(lane & 31u));
                    const float ao = aq_of[qb];
                    uint32_t m = 0;
#pragma unroll
                    for (uint32_t v4 = 0; v4 < 4u; ++v4) {
                        const uint32_t rbase = 8u * v4 + 4u * (lane >> 5);
                        const float4 t01 = bterm[rbase / 2u];
                        const float4 t23 = bterm[rbase / 2u + 1u];
                        const float ad[4] = {t01.x, t01.z, t23.x, t23.z}, ed[4] = {t01.y, t01.w, t23.y, t23.w};
#pragma unroll
                        for (uint32_t i = 0; i < 4u; ++i) {
                            const float g = (ao + ad[i]) - 2.0f * acc[qb][4u * v4 + i];
                            const float y = xo + ed[i];
                            m |= g > y * y ? 1u << (rbase + i) : 0u;
                        }
                    }
                    rej[qb] = m;
                }
                // a query's rows lie in lanes l and l ^ 32 of its set: send the other set's word across, keep the own one
                const uint32_t other = (uint32_t)__shfl_xor((int)(lane < 32u ? rej[1] : rej[0]), 32);
                need = want & ~((lane < 32u ? rej[0] : rej[1]) | other);
            }
            nexact += (uint32_t)__popc(need);
            // the exact step: every lane with a row left takes its lowest one, from D by id, through the admission sequence of
            // hvs_scan_rows_into_lists
            while (__ballot(need != 0u) != 0ull) {
                const bool on = need != 0u;
                const uint32_t r = on ? (uint32_t)__builtin_ctz(need) : 0u;
                need &= need - 1u;
                const uint32_t id = bid[r];
                float dist = 0.0f;
                if (on) {
                    const float* __restrict__ dv = D + (size_t)id * HVS_DCOLS + 2;
                    if (SCALAR_ORDER)
                        dist = hvs_scalar_order_dist(dv, qrow + 4);
                    else
                        dist = hvs_exact_dist_pk(reinterpret_cast<const hvs_f2*>(dv), reinterpret_cast<const hvs_f2*>(qrow + 4));
                }
                bool adm = on && takes && !(dist > tau);
                if constexpr (AFTER) adm = adm && hvs_make_key(dist, id) >= key_lo;
                if constexpr (EXCL) {
                    if (adm && hvs_refuse_listed(excl, qi, id)) adm = false;
                }
                // a key that finds its segment full: the wave cuts the segment first (or flags the query when it cannot)
                uint64_t full = __ballot(adm && cnt == segcap);
                if (full != 0ull) {
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                    while (full != 0ull) {
                        const uint32_t l = (uint32_t)__builtin_ctzll(full);
                        full &= full - 1ull;
                        const uint32_t lcap = (uint32_t)__shfl((int)segcap, (int)l);
                        if (lcap <= knn) {  // no room to cut in: the query is run again (larger lists, or the exact engine)
                            if (lane == l) {
                                hvs_flag_fail(B.fail_code, B.overflow, slot);
                                takes = false;
                            }
                            continue;
                        }
                        const uint32_t ls0 = (uint32_t)__shfl((int)s0, (int)l);
                        uint64_t* lst = O.lists + (size_t)(w * 64u + l) * O.stride + ls0;
                        const uint64_t kth = hvs_wave_select_prune<CAP / 64>(lst, lcap, knn, lane);
                        if (lane == l) {
                            cnt = knn;
                            tau = fminf(tau, hvs_key_dist(kth));  // (a NaN key leaves tau as it is)
                        }
                    }
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                    adm = adm && takes && !(dist > tau);  // (against the threshold the cut has just set)
                }
                if (adm) {
                    myseg[cnt] = hvs_make_key(dist, id);
                    ++cnt;
                    ++nadm;
                }
            }
        }
        hvs_stage_barrier();
        buf ^= 1u;
    }
    if (owns) O.counts[slot] = s0 + cnt;
    if constexpr (EXCL) {
        if (wave_active) hvs_count_refused(lane, counters);  // (wave-uniform)
    }
    if (count && wave_active) {
        // npass, nadm and nexact are per lane; the rows seen and the rows bounded per wave, times the wave's queries
        const uint64_t hm = __ballot(have_q);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            npass += __shfl_xor(npass, o);
            nadm += __shfl_xor(nadm, o);
            nexact += __shfl_xor(nexact, o);
        }
        if (lane == 0u && hm != 0ull) {
            const unsigned long long nhave = (unsigned long long)__popcll(hm);
            atomicAdd(&counters[HVS_CNT_PAIRS], (unsigned long long)npass);
            atomicAdd(&counters[CNT], (unsigned long long)nrows_seen * nhave);
            if (nadm) atomicAdd(&counters[CNT + 1], (unsigned long long)nadm);
            if (nbound) atomicAdd(&counters[HVS_CNT_BEHIND_BOUND], (unsigned long long)nbound * nhave);
            if (nexact) atomicAdd(&counters[HVS_CNT_BEHIND_EXACT], (unsigned long long)nexact);
        }
    }
}
