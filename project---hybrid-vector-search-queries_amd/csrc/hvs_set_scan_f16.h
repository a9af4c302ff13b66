// hvs_set_scan_f16.h -- scanned row sets with an FP16 MFMA bound in front of the exact distance.
// hvs_k_scan_set_members_f16 is hvs_k_scan_set_members (hvs_set_scan.h) with one more step inside a staged block of rows: a
// matrix product of the block's rows and the wave's 64 queries, both rounded to IEEE half, gives every (query, row) pair a
// LOWER BOUND on the reference's f32 distance, and a pair whose bound lies above the lane's threshold is never evaluated.
// Whatever is evaluated goes through the functions, the operands and the admission sequence of the unfiltered kernel, rows
// ascending per lane, so a lane's keys and its history of thresholds are that kernel's and the partial lists match word for
// word.  Same items, same lists, same merge (hvs_k_merge_set_chunks); chosen by hvs_set_row_set_scan_filter(ctx, 1).
//
// The bound.  d^ = half(d) as the matrix pipe uses it, e_d >= |d - d^|, N_d = |d^|^2, likewise for q; s~ the pipe's q^.d^.
//   |q - d| >= |q^ - d^| - e_q - e_d                                           (triangle)
//   |q^ - d^|^2 = N_q + N_d - 2 q^.d^ >= N_q + N_d - 2 s~ - 2 mu,   mu = 256 u |q^| |d^| <= 128 u (N_q + N_d), u = 2^-24
//   R >= T (1 - g) - 1e-30,  T = |q - d|^2                                      (g: f32 roundings of the reference order)
// so with G = A_q + A_d - 2 s~ (A_x = N_x (1 - kappa) rounded down, kappa = 272 u: 2 mu and the f32 evaluation of G itself)
// and X = e_q + sqrt((thr + 1e-30)(1 + 2 g)) rounded up, a pair with G > (X + e_d)^2 has R > thr, and thr = tau (or the cap if
// that is lower) refuses it.  A flush of half subnormals in the pipe is inside e_x (HVS_F16_FLUSH on each) and N_x (8e-7 on
// A_q).  A row or query with a component that is not finite as a half has A_x = NaN: G is NaN, the comparison is false, the
// pair is evaluated.  While tau is NaN and no cap is attached X is NaN and every passing row is evaluated.
#pragma once

#include "hvs_filter.h"
#include "hvs_set_scan.h"

#define HVS_SCANF_ROWS 32u      // rows per staged block: the M of v_mfma_f32_32x32x16_f16
#define HVS_SCANF_ROW_F 108u    // floats per staged f32 row: 4 * 27, so that 16 consecutive rows start in 16 different bank quads
#define HVS_SCANF_KSTEPS 7u     // K = 100 padded with zeros to 112 = 7 steps of 16
#define HVS_SCANF_UP 1.0000153f      // 1 + 2^-16: over the f32 summation error of a 100-term sum of squares (105 u)
#define HVS_SCANF_A 0.9999684f       // below 1 - 2^-16 - 272 u (1 + 2^-10) = 0.99996851..
#define HVS_SCANF_TINY 1.0000010f    // 1 + 2^-20: over the three roundings of (X + e_d)^2 and of a square root

// (e^2, n^2) of four components: n = the half nearest to x, e = x - n (exact in f32)
__device__ __forceinline__ float2 hvs_scanf_part(const float4& v, hvs_f2& h01, hvs_f2& h23)
{
    const float n0 = (float)(_Float16)v.x, n1 = (float)(_Float16)v.y, n2 = (float)(_Float16)v.z, n3 = (float)(_Float16)v.w;
    const float e0 = v.x - n0, e1 = v.y - n1, e2 = v.z - n2, e3 = v.w - n3;
    h01 = hvs_f2{n0, n1};
    h23 = hvs_f2{n2, n3};
    return make_float2((e0 * e0 + e1 * e1) + (e2 * e2 + e3 * e3), (n0 * n0 + n1 * n1) + (n2 * n2 + n3 * n3));
}
__device__ __forceinline__ uint32_t hvs_scanf_pack(const hvs_f2& h)
{
    return (uint32_t)hvs_f16_bits(h.x) | ((uint32_t)hvs_f16_bits(h.y) << 16);
}
// (A_x, e_x) from the sums (e^2, n^2); `flush_n`: what a flush of subnormals can take from N_x (the query carries both sides')
__device__ __forceinline__ float2 hvs_scanf_terms(float e2, float n2, float flush_n)
{
    const bool ok = e2 < __builtin_inff() && n2 < __builtin_inff();
    const float a = n2 * HVS_SCANF_A - flush_n;
    const float e = (sqrtf(e2 * HVS_SCANF_UP) * HVS_SCANF_TINY + (float)(HVS_F16_FLUSH + 1e-9)) * HVS_SCANF_TINY;
    return make_float2(ok ? a : __builtin_nanf(""), e);
}

// Budget: ONE workgroup per CU, one wave per SIMD, so that a lane may use the whole unified file of 512 registers: the query's
// 100 floats, 56 registers of its half fragments, 32 accumulators, 20 of staging and the row data of the exact step in flight.
// At two workgroups per CU (256 registers) the compiler spilled some 260 registers to scratch, which this kernel must not use.
// LDS 58.6 KB a workgroup: 2 x 13.5 KB f32 rows, 2 x 7 KB half fragments, 2 x 6.25 KB partial norms, 4 KB select histograms,
// 1 KB per-row terms.
template <bool SCALAR_ORDER, int CAP>
__global__ __launch_bounds__(256, 1) void hvs_k_scan_set_members_f16(
    const float* __restrict__ D, uint32_t sn, const float* __restrict__ Q, const uint32_t* __restrict__ order,
    const HvsScanItem* __restrict__ items, const uint32_t* __restrict__ mem_off, const uint32_t* __restrict__ members,
    const uint32_t* __restrict__ live, const float* __restrict__ caps, const uint64_t* __restrict__ after_lo, HvsExcl excl,
    uint64_t* __restrict__ lists, uint32_t* __restrict__ list_cnt, uint32_t knn, unsigned long long* __restrict__ counters)
{
    constexpr uint32_t RB = HVS_SCANF_ROWS, RF4 = HVS_SCANF_ROW_F / 4u, KS = HVS_SCANF_KSTEPS;
    __shared__ float4 srow[2][RB * RF4];       // f32 rows: 25 pieces of 4 floats, then (C, T, id, -)
    __shared__ __attribute__((aligned(16))) uint2 shalf[2][KS * 64u * 2u];  // the A operand: k-step ks, lane l = (row l & 31, k = 16 ks + 8 (l >> 5) + 0..7), 2 x 8 bytes
    __shared__ float2 spart[2][RB * 25u];      // (e^2, n^2) of every piece of 4 floats
    __shared__ __attribute__((aligned(16))) float2 sterm[4][RB];  // per wave: (A_d, e_d) of the block's rows
    __shared__ uint32_t shist[4][256];         // digit histograms of the radix select
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
    // the lane's own query: A_q, e_q in the fixed order of the components
    float aq, eq;
    {
        float e2 = 0.0f, n2 = 0.0f;
#pragma unroll
        for (int i = 0; i < HVS_NDIM / 4; ++i) {
            hvs_f2 h01, h23;
            const float2 s = hvs_scanf_part(make_float4(q2[2 * i].x, q2[2 * i].y, q2[2 * i + 1].x, q2[2 * i + 1].y), h01, h23);
            e2 += s.x;
            n2 += s.y;
        }
        const float2 t = hvs_scanf_terms(e2, n2, 8e-7f);
        aq = t.x;
        eq = t.y;
    }
    // the B operand, in registers: set qb holds queries 32 qb .. 32 qb + 31 of the wave; lane l of k-step ks carries query column
    // l & 31, k = 16 ks + 8 (l >> 5) + 0..7.  Read once per item from the query rows (the other lane's row: its index by shuffle).
    hvs_f16x8 bq[2][KS];
    float aq_of[2];
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
        const int src = qb * 32 + (int)(lane & 31u);
        const uint32_t qo = (uint32_t)__shfl((int)qi, src);
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
    const uint32_t* __restrict__ mem = members + mem_off[it.set];
    const uint32_t m0 = it.m_begin, m1 = it.m_end;

    // staging: piece e = (row r, part c): c < 25 -> floats 2+4c..5+4c of the row, c == 25 -> (C, T, id, 0)
    constexpr uint32_t kItems = RB * 26u;
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
    // the f32 piece, and for c < 25 its four halves in the operand layout and its partial norms; the thread of the attribute
    // piece writes the zeros of k = 100..111 (the 8-byte slots 25, 26, 27 of the row)
    auto half_slot = [&](uint32_t r, uint32_t c) { return ((c >> 2) * 64u + ((c >> 1) & 1u) * 32u + r) * 2u + (c & 1u); };
    auto store_block = [&](uint32_t buf) {
#pragma unroll
        for (uint32_t k = 0; k < kPer; ++k) {
            const uint32_t e = threadIdx.x + 256u * k;
            if (e < kItems) {
                const uint32_t r = e / 26u, c = e % 26u;
                srow[buf][r * RF4 + c] = stg[k];
                if (c < 25u) {
                    hvs_f2 h01, h23;
                    spart[buf][r * 25u + c] = hvs_scanf_part(stg[k], h01, h23);
                    shalf[buf][half_slot(r, c)] = make_uint2(hvs_scanf_pack(h01), hvs_scanf_pack(h23));
                } else {
                    shalf[buf][half_slot(r, 25u)] = make_uint2(0u, 0u);
                    shalf[buf][half_slot(r, 26u)] = make_uint2(0u, 0u);
                    shalf[buf][half_slot(r, 27u)] = make_uint2(0u, 0u);
                }
            }
        }
    };

    uint64_t* __restrict__ mylist = lists + (size_t)(it.slot + threadIdx.x) * CAP;
    float tau = __builtin_nanf("");  // (NaN until the segment has been cut once: `!(dist >= tau)` admits every passing row)
    const float cap = caps ? caps[qi] : 0.0f;
    const uint64_t lo = after_lo ? after_lo[qi] : 0ull;
    const float g2 = 1.0f + 2.0f * (SCALAR_ORDER ? 104.0f : 20.0f) * 5.9604644775390625e-08f;  // 1 + 2 g (sequential order: 104 roundings)
    uint32_t cnt = 0, npass = 0, nbound = 0, nexact = 0;

    load_ids(m0);
    load_block();
    load_ids(m0 + RB);
    store_block(0u);
    __syncthreads();
    uint32_t buf = 0;
    for (uint32_t j0 = m0; j0 < m1; j0 += RB) {
        const bool more = j0 + RB < m1;
        if (more) {
            load_block();           // rows of the next block, by the ids fetched a block ago
            load_ids(j0 + 2u * RB);  // ids of the block after it
        }
        if (wave_active) {
            const uint32_t nrow = (m1 - j0) < RB ? (m1 - j0) : RB;
            // which rows count (wave-uniform: in the prefix, live) and which of them this lane's query wants
            uint32_t valid = 0, want = 0;
            for (uint32_t r = 0; r < nrow; ++r) {
                const float4 attr = srow[buf][r * RF4 + 25u];
                const uint32_t id = __builtin_amdgcn_readfirstlane(__float_as_uint(attr.z));
                if (!(id < sn)) continue;                                   // (wave-uniform)
                if (live != nullptr && !hvs_row_live(live, id)) continue;  // (wave-uniform)
                valid |= 1u << r;
                want |= hvs_row_passes(p, attr.x, attr.y) ? 1u << r : 0u;
            }
            npass += (uint32_t)__popc(want);
            // the lane's threshold as X' = (e_q + sqrt((thr + 1e-30)(1 + 2g))) rounded up; NaN or +inf: nothing is refused
            const float thr = caps != nullptr ? fminf(tau, cap) : tau;
            const float x = (eq + sqrtf((thr + 1e-30f) * g2 * HVS_SCANF_TINY) * HVS_SCANF_TINY) * HVS_SCANF_TINY;
            uint32_t need = want;
            if (__ballot(want != 0u && x < __builtin_inff()) != 0ull) {  // (wave-uniform) some lane can refuse something
                nbound += (uint32_t)__popc(valid);
                // per-row terms: lane l sums the partial norms of row l & 31, pieces 13 (l >> 5) .., in order; the halves meet by shuffle
                {
                    const uint32_t r = lane & 31u, c0 = 13u * (lane >> 5), c1 = c0 ? 25u : 13u;
                    float e2 = 0.0f, n2 = 0.0f;
                    for (uint32_t c = c0; c < c1; ++c) {
                        const float2 s = spart[buf][r * 25u + c];
                        e2 += s.x;
                        n2 += s.y;
                    }
                    e2 += __shfl_xor(e2, 32);
                    n2 += __shfl_xor(n2, 32);
                    const float2 t = hvs_scanf_terms(e2, n2, 0.0f);
                    if (lane < 32u) sterm[w][r] = make_float2(t.x, t.y * HVS_SCANF_TINY);
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                }
                hvs_f32x16 acc[2];
#pragma unroll
                for (int qb = 0; qb < 2; ++qb)
#pragma unroll
                    for (int v = 0; v < 16; ++v) acc[qb][v] = 0.0f;
#pragma unroll
                for (uint32_t ks = 0; ks < KS; ++ks) {
                    const uint4 au = *reinterpret_cast<const uint4*>(&shalf[buf][(ks * 64u + lane) * 2u]);
                    const hvs_f16x8 a = HvsFmt<HVS_FMT_F16>::frag(au);
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bq[0][ks], acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bq[1][ks], acc[1], 0, 0, 0);
                }
                // accumulator v of a lane is row (v & 3) + 8 (v >> 2) + 4 (l >> 5) of query column l & 31 of its set
                uint32_t rej[2];
#pragma unroll
                for (int qb = 0; qb < 2; ++qb) {
                    const float xo = __shfl(x, qb * 32 + (int)(lane & 31u));
                    const float ao = aq_of[qb];
                    uint32_t m = 0;
#pragma unroll
                    for (uint32_t v4 = 0; v4 < 4u; ++v4) {
                        const uint32_t rbase = 8u * v4 + 4u * (lane >> 5);
                        const float4 t01 = *reinterpret_cast<const float4*>(&sterm[w][rbase]);
                        const float4 t23 = *reinterpret_cast<const float4*>(&sterm[w][rbase + 2u]);
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
            // the exact step: every lane with a row left takes its lowest one
            while (__ballot(need != 0u) != 0ull) {
                const bool on = need != 0u;
                const uint32_t r = on ? (uint32_t)__builtin_ctz(need) : 0u;
                need &= need - 1u;
                const float4* rowp = &srow[buf][r * RF4];
                const uint32_t id = __float_as_uint(rowp[25].z);
                float dist;
                if (SCALAR_ORDER) {
                    const HvsLdsRow1 d1{reinterpret_cast<const float*>(rowp)};
                    const HvsPairAsScalar q1{q2};
                    dist = hvs_scalar_order_dist(d1, q1);
                } else {
                    dist = hvs_exact_dist_pk_lds(rowp, q2);
                }
                bool admit = on && !(dist >= tau);
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
    if (wave_active) {
        // npass and nexact are per lane, nbound per wave (rows) times the wave's queries
        const uint32_t nhave = (uint32_t)__popcll(__ballot(have_q));
        unsigned long long sp = npass, sx = nexact;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            sp += (unsigned long long)__shfl_xor((long long)sp, o);
            sx += (unsigned long long)__shfl_xor((long long)sx, o);
        }
        if (lane == 0u) {
            if (sp) atomicAdd(&counters[HVS_CNT_PAIRS], sp);
            if (nbound) atomicAdd(&counters[HVS_CNT_SCANNED], (unsigned long long)nbound * nhave);
            if (sx) atomicAdd(&counters[HVS_CNT_RESCORED], sx);
        }
    }
}

template <bool SCALAR_ORDER, int CAP>
static inline void hvs_launch_set_scan_f16_as(hipStream_t stream, uint32_t n_items, const HvsSetScanArgs& a)
{
    const HvsExcl excl{a.ex_begin, a.ex_count, a.ex_ids, nullptr, nullptr, 0u, 0u};
    hipLaunchKernelGGL((hvs_k_scan_set_members_f16<SCALAR_ORDER, CAP>), dim3(n_items), dim3(256), 0, stream, a.D, a.sn, a.Q, a.order, a.items, a.mem_off,
                       a.members, a.live, a.caps, a.after_lo, excl, a.lists, a.list_cnt, a.knn, a.counters);
}
// The one launch site's call.  filter 0: hvs_launch_set_scan, what every call launched before.  filter 1: the filtered scan over
// the same items, then the same merge (hvs_launch_set_scan without items launches the merge alone).
static inline void hvs_launch_set_scan_by(hipStream_t stream, uint32_t filter, bool scalar_order, int cap, uint32_t n_items, const HvsSetScanArgs& a)
{
    if (filter == 0u) return hvs_launch_set_scan(stream, scalar_order, cap, n_items, a);
    if (n_items) {
        if (cap == 512)
            scalar_order ? hvs_launch_set_scan_f16_as<true, 512>(stream, n_items, a) : hvs_launch_set_scan_f16_as<false, 512>(stream, n_items, a);
        else
            scalar_order ? hvs_launch_set_scan_f16_as<true, 256>(stream, n_items, a) : hvs_launch_set_scan_f16_as<false, 256>(stream, n_items, a);
    }
    hvs_launch_set_scan(stream, scalar_order, cap, 0u, a);
}
