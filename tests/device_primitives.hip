// device_primitives.hip -- the wave-level device primitives of csrc/hvs_device.h and csrc/hvs_kernels.h, each run on its own
// against cases that tests/primitives_model.py writes and models (tests/test_primitives.py, tests/test_primitives_cpu.py).
//
//   device_primitives.out CASES RESULTS
//
// CASES and RESULTS are blob files: u32 words [magic, nblobs, (offset, length) x nblobs, data ...], offsets and lengths in
// words, every blob 8-byte aligned.  The blob numbers are the enums below; primitives_model.py holds the same lists by name.
// Every section launches as the real kernels do: 256-thread workgroups of four waves, one case per wave, a CAP-key LDS buffer
// and a 256-word histogram per wave.  One process, every launch once, in a fixed order; any HIP error ends the run non-zero
// before another launch starts.  One line per section on stdout.
//
// Built with engine.HIPCC_FLAGS minus -shared and -fPIC: -ffp-contract=off is what the distance section is about.
#include <hip/hip_runtime.h>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../project---hybrid-vector-search-queries_amd/csrc/hvs_kernels.h"

enum InBlob : int {
    IN_SEL4_DESC, IN_SEL4_LISTS, IN_SEL8_DESC, IN_SEL8_LISTS,
    IN_CUT256_DESC, IN_CUT256_LISTS, IN_CUT512_DESC, IN_CUT512_LISTS,
    IN_PAD_DESC, IN_PAD_LISTS, IN_PAD_TAB, IN_PAD_D, IN_PAD_QX,
    IN_RANK_DESC, IN_RANK_KEYS, IN_RANK_OUTLEN,
    IN_KEEP_DESC, IN_KEEP_LISTS, IN_KEEP_NGROUPS, IN_EXCL_CFG, IN_EXCL_POOL, IN_EXQ_DESC, IN_SETQ_DESC,
    IN_GATH256_DESC, IN_GATH256_LISTS, IN_GATH512_DESC, IN_GATH512_LISTS, IN_GATH_IDS, IN_GATH_DISTS,
    IN_DEDUP256_DESC, IN_DEDUP256_LISTS, IN_DEDUP512_DESC, IN_DEDUP512_LISTS,
    IN_DIST_D, IN_DIST_Q,
    IN_PRED_Q, IN_PRED_ROWS, IN_ORD_F,
    IN_COUNT
};
enum OutBlob : int {
    // select: [NK = 4, 8][form: histogram compact, histogram no compact, bit-serial LDS, bit-serial global] x (lists, kth)
    OUT_SEL = 0,
    OUT_CUT256_LISTS = 16, OUT_CUT256_RET, OUT_CUT256_KTH, OUT_CUT512_LISTS, OUT_CUT512_RET, OUT_CUT512_KTH,
    OUT_PAD_LISTS, OUT_RANK_IDS, OUT_RANK_DISTS,
    OUT_KEEP_LISTS, OUT_KEEP_RET, OUT_KEEP_COUNTERS, OUT_EXQ, OUT_SETQ,
    OUT_GATH256_LISTS, OUT_GATH256_RET, OUT_GATH512_LISTS, OUT_GATH512_RET,
    OUT_DEDUP256_LISTS, OUT_DEDUP256_RET, OUT_DEDUP512_LISTS, OUT_DEDUP512_RET,
    OUT_DIST_PLAIN, OUT_DIST_PK, OUT_DIST_LDS, OUT_DIST_SCALAR,
    OUT_PRED_PARAMS, OUT_PRED_PASS, OUT_ORD,
    OUT_COUNT
};
#define HVP_MAGIC 0x50535648u
#define HVP_KTH_UNTOUCHED 0x0DDBA11500C0FFEEull  // what a kth out-parameter holds where nothing wrote it
#define HVP_PAD_CAP 256
#define HVP_KEEP_CAP 512

#define CHECK(x)                                                                                          \
    do {                                                                                                  \
        const hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) {                                                                           \
            fprintf(stderr, "HIP error %d (%s) at %s:%d: %s\n", (int)e_, hipGetErrorString(e_), __FILE__, __LINE__, #x); \
            exit(2);                                                                                      \
        }                                                                                                 \
    } while (0)

// ------------------------------------------------------------------------------------------------------------ device side
template <int CAP>
__device__ __forceinline__ void hvp_load(uint64_t* buf, const uint64_t* __restrict__ src, uint32_t lane)
{
    for (uint32_t e = lane; e < (uint32_t)CAP; e += 64u) buf[e] = src[e];
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
}
template <int CAP>
__device__ __forceinline__ void hvp_store(const uint64_t* buf, uint64_t* __restrict__ dst, uint32_t lane)
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    for (uint32_t e = lane; e < (uint32_t)CAP; e += 64u) dst[e] = buf[e];
}

// desc: [cnt, keep] per case.  FORM 3 works in place on out (the host copied the lists there).
template <int NK, int FORM>
__global__ __launch_bounds__(256) void hvp_k_select(const uint32_t* __restrict__ desc, uint32_t ncases, const uint64_t* __restrict__ in,
                                                    uint64_t* out, uint64_t* __restrict__ kth)
{
    constexpr int CAP = 64 * NK;
    __shared__ uint64_t sbuf[4][CAP];
    __shared__ uint32_t shist[4][256];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t c = blockIdx.x * 4u + w;
    if (c >= ncases) return;  // wave-uniform
    const uint32_t cnt = desc[2u * c], keep = desc[2u * c + 1u];
    uint64_t* buf = sbuf[w];
    uint64_t k;
    if constexpr (FORM == 3) {
        k = hvs_wave_select_prune<NK>(out + (size_t)c * CAP, cnt, keep, lane);
    } else {
        hvp_load<CAP>(buf, in + (size_t)c * CAP, lane);
        if constexpr (FORM == 0) k = hvs_wave_select_prune<NK, true>(buf, cnt, keep, lane, shist[w]);
        if constexpr (FORM == 1) k = hvs_wave_select_prune<NK, false>(buf, cnt, keep, lane, shist[w]);
        if constexpr (FORM == 2) k = hvs_wave_select_prune<NK>(buf, cnt, keep, lane);
        hvp_store<CAP>(buf, out + (size_t)c * CAP, lane);
    }
    if (lane == 0u) kth[c] = k;
}

// desc: [cnt, step, knn, op] per case; op 0: make_room with kth, 1: make_room without, 2: final_cut (step unused)
template <int CAP>
__global__ __launch_bounds__(256) void hvp_k_cut(const uint32_t* __restrict__ desc, uint32_t ncases, const uint64_t* __restrict__ in,
                                                 uint64_t* __restrict__ out, uint32_t* __restrict__ ret, uint64_t* __restrict__ kth)
{
    __shared__ uint64_t sbuf[4][CAP];
    __shared__ uint32_t shist[4][256];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t c = blockIdx.x * 4u + w;
    if (c >= ncases) return;
    const uint32_t cnt = desc[4u * c], step = desc[4u * c + 1u], knn = desc[4u * c + 2u], op = desc[4u * c + 3u];
    uint64_t* buf = sbuf[w];
    hvp_load<CAP>(buf, in + (size_t)c * CAP, lane);
    uint64_t kk = HVP_KTH_UNTOUCHED;
    uint32_t r;
    if (op == 0u)
        r = hvs_wave_make_room<CAP>(buf, shist[w], cnt, step, knn, lane, &kk);
    else if (op == 1u)
        r = hvs_wave_make_room<CAP>(buf, shist[w], cnt, step, knn, lane);
    else
        r = hvs_wave_final_cut<CAP>(buf, shist[w], cnt, knn, lane);
    hvp_store<CAP>(buf, out + (size_t)c * CAP, lane);
    if (lane == 0u) {
        ret[c] = r;
        kth[c] = kk;
    }
}

// desc: [cnt, knn, pad, mode, tab_off, qa, qb, n_rows] per case.  mode 0: key_of(s) = tab[tab_off + s]; 1 / 2: hvs_row_key of row
// n_rows - 1 - s against query row qa of Qx in the SIMD / the sequential order; 3 / 4: hvs_row_key_min over query rows [qa, qb)
__global__ __launch_bounds__(256) void hvp_k_pad(const uint32_t* __restrict__ desc, uint32_t ncases, const uint64_t* __restrict__ in,
                                                 const uint64_t* __restrict__ tab, const float* __restrict__ D, const float* __restrict__ Qx,
                                                 uint64_t* __restrict__ out)
{
    constexpr int CAP = HVP_PAD_CAP;
    __shared__ uint64_t sbuf[4][CAP];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t c = blockIdx.x * 4u + w;
    if (c >= ncases) return;
    const uint32_t* d = desc + 8u * c;
    const uint32_t cnt = d[0], knn = d[1], mode = d[3], tab_off = d[4], qa = d[5], qb = d[6], n = d[7];
    const int pad = (int)d[2];
    uint64_t* buf = sbuf[w];
    hvp_load<CAP>(buf, in + (size_t)c * CAP, lane);
    const float* qv = Qx + (size_t)qa * HVS_QCOLS + 4;
    if (mode == 0u)
        hvs_wave_pad(buf, cnt, knn, pad, lane, [=](uint32_t s) { return tab[tab_off + s]; });
    else if (mode == 1u)
        hvs_wave_pad(buf, cnt, knn, pad, lane, [=](uint32_t s) { return hvs_row_key<false>(D, n - 1u - s, qv); });
    else if (mode == 2u)
        hvs_wave_pad(buf, cnt, knn, pad, lane, [=](uint32_t s) { return hvs_row_key<true>(D, n - 1u - s, qv); });
    else if (mode == 3u)
        hvs_wave_pad(buf, cnt, knn, pad, lane, [=](uint32_t s) { return hvs_row_key_min<false>(D, n - 1u - s, Qx, qa, qb); });
    else
        hvs_wave_pad(buf, cnt, knn, pad, lane, [=](uint32_t s) { return hvs_row_key_min<true>(D, n - 1u - s, Qx, qa, qb); });
    hvp_store<CAP>(buf, out + (size_t)c * CAP, lane);
}

// desc: [knn, with_dists, row, key_off] per case: keys[key_off .. key_off + knn) to result row `row` of knn slots
__global__ __launch_bounds__(256) void hvp_k_rank(const uint32_t* __restrict__ desc, uint32_t ncases, const uint64_t* __restrict__ keys,
                                                  uint32_t* __restrict__ out_ids, float* __restrict__ out_dists)
{
    constexpr int CAP = HVP_PAD_CAP;
    __shared__ uint64_t sbuf[4][CAP];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t c = blockIdx.x * 4u + w;
    if (c >= ncases) return;
    const uint32_t knn = desc[4u * c], with = desc[4u * c + 1u], row = desc[4u * c + 2u], off = desc[4u * c + 3u];
    uint64_t* buf = sbuf[w];
    for (uint32_t e = lane; e < knn; e += 64u) buf[e] = keys[off + e];
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    hvs_wave_rank_write(buf, knn, lane, row, out_ids, with ? out_dists : nullptr);
}

struct HvpExclCfg {  // offsets into the u32 pool; set_of_off 0xFFFFFFFF: no set_of
    uint32_t begin_off, count_off, ids_off, set_of_off, set_bits_off, set_words, row0, unused;
};
__device__ __forceinline__ HvsExcl hvp_excl(const uint32_t* __restrict__ cfgs, uint32_t i, const uint32_t* __restrict__ pool)
{
    const uint32_t* c = cfgs + 8u * i;
    HvsExcl x;
    x.begin = pool + c[0];
    x.count = pool + c[1];
    x.ids = pool + c[2];
    x.set_of = c[3] == 0xFFFFFFFFu ? nullptr : pool + c[3];
    x.set_bits = pool + c[4];
    x.set_words = c[5];
    x.row0 = c[6];
    return x;
}

// desc: [fn, cnt, knn, count, group, p0, p1, unused] per case.  fn 0: hvs_keep_within, cap = bits p0; 1: hvs_keep_after, lo = p1:p0;
// 2: hvs_keep_unlisted with HvsExcl configuration p0 and query p1.  Counters: block `group` of HVS_CNT_COUNT words.
__global__ __launch_bounds__(256) void hvp_k_keep(const uint32_t* __restrict__ desc, uint32_t ncases, const uint64_t* __restrict__ in,
                                                  const uint32_t* __restrict__ cfgs, const uint32_t* __restrict__ pool,
                                                  uint64_t* __restrict__ out, uint32_t* __restrict__ ret, unsigned long long* __restrict__ ctr)
{
    constexpr int CAP = HVP_KEEP_CAP;
    __shared__ uint64_t sbuf[4][CAP];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t c = blockIdx.x * 4u + w;
    if (c >= ncases) return;
    const uint32_t* d = desc + 8u * c;
    const uint32_t fn = d[0], cnt = d[1], knn = d[2];
    const bool count = d[3] != 0u;
    unsigned long long* counters = ctr + (size_t)d[4] * HVS_CNT_COUNT;
    uint64_t* buf = sbuf[w];
    hvp_load<CAP>(buf, in + (size_t)c * CAP, lane);
    uint32_t r;
    if (fn == 0u) {
        r = hvs_keep_within(buf, cnt, __uint_as_float(d[5]), knn, lane, counters, count);
    } else if (fn == 1u) {
        r = hvs_keep_after(buf, cnt, ((uint64_t)d[6] << 32) | d[5], knn, lane, counters, count);
    } else {
        const HvsExcl x = hvp_excl(cfgs, d[5], pool);
        r = hvs_keep_unlisted(buf, cnt, x, d[6], knn, lane, counters, count);
    }
    hvp_store<CAP>(buf, out + (size_t)c * CAP, lane);
    if (lane == 0u) ret[c] = r;
}

// one thread per pair.  desc: [list_off, count, id, unused]
__global__ void hvp_k_excluded(const uint32_t* __restrict__ desc, uint32_t n, const uint32_t* __restrict__ pool, uint32_t* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = hvs_excluded(pool + desc[4u * i], desc[4u * i + 1u], desc[4u * i + 2u]) ? 1u : 0u;
}
// desc: [cfg, qi, id, unused]
__global__ void hvp_k_in_row_set(const uint32_t* __restrict__ desc, uint32_t n, const uint32_t* __restrict__ cfgs,
                                 const uint32_t* __restrict__ pool, uint32_t* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const HvsExcl x = hvp_excl(cfgs, desc[4u * i], pool);
    out[i] = hvs_in_row_set(x, desc[4u * i + 1u], desc[4u * i + 2u]) ? 1u : 0u;
}

// desc: [cnt0, knn, ids_off, dists_off, row0 low, row0 high, unused, unused]
template <int CAP>
__global__ __launch_bounds__(256) void hvp_k_gather(const uint32_t* __restrict__ desc, uint32_t ncases, const uint64_t* __restrict__ in,
                                                    const uint32_t* __restrict__ ids, const float* __restrict__ dists,
                                                    uint64_t* __restrict__ out, uint32_t* __restrict__ ret)
{
    __shared__ uint64_t sbuf[4][CAP];
    __shared__ uint32_t shist[4][256];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t c = blockIdx.x * 4u + w;
    if (c >= ncases) return;
    const uint32_t* d = desc + 8u * c;
    uint64_t* buf = sbuf[w];
    hvp_load<CAP>(buf, in + (size_t)c * CAP, lane);
    const uint32_t r = hvs_gather_list_keys<CAP>(buf, shist[w], d[0], ids + d[2], dists + d[3], ((uint64_t)d[5] << 32) | d[4], d[1], lane);
    hvp_store<CAP>(buf, out + (size_t)c * CAP, lane);
    if (lane == 0u) ret[c] = r;
}

// desc: [cnt, unused]
template <int CAP>
__global__ __launch_bounds__(256) void hvp_k_dedup(const uint32_t* __restrict__ desc, uint32_t ncases, const uint64_t* __restrict__ in,
                                                   uint64_t* __restrict__ out, uint32_t* __restrict__ ret)
{
    __shared__ uint64_t sbuf[4][CAP];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t c = blockIdx.x * 4u + w;
    if (c >= ncases) return;
    uint64_t* buf = sbuf[w];
    hvp_load<CAP>(buf, in + (size_t)c * CAP, lane);
    const uint32_t r = hvs_wave_dedup_ids<CAP>(buf, desc[2u * c], lane);
    hvp_store<CAP>(buf, out + (size_t)c * CAP, lane);
    if (lane == 0u) ret[c] = r;
}

// The four distance forms on pair p = (row p of D, row p of Q), 100 floats each; one lane per pair, 64 pairs per wave.  The LDS
// form as the scan runs it: the lane's query in registers as 50 pairs, the row staged in the wave's HVS_LDS_ROW_F image
// [x0..x99, C, T, pad, pad] and read back by every lane; the wave stages its 64 rows one after another and lane r keeps row r's.
__global__ __launch_bounds__(256) void hvp_k_dist(const float* __restrict__ D, const float* __restrict__ Q, uint32_t npairs,
                                                  uint64_t* __restrict__ o_plain, uint64_t* __restrict__ o_pk, uint64_t* __restrict__ o_lds,
                                                  uint64_t* __restrict__ o_scalar)
{
    __shared__ float4 srow[4][HVS_LDS_ROW_F / 4];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t p0 = (blockIdx.x * 4u + w) * 64u;
    if (p0 >= npairs) return;  // wave-uniform
    const uint32_t last = npairs - 1u;
    const uint32_t p = p0 + lane < last ? p0 + lane : last;
    const float* d = D + (size_t)p * HVS_NDIM;
    const float* q = Q + (size_t)p * HVS_NDIM;
    const float plain = hvs_exact_dist(d, q);
    const float pk = hvs_exact_dist_pk((const hvs_f2*)d, (const hvs_f2*)q);
    const float scalar = hvs_scalar_order_dist(d, q);
    hvs_f2 q2[50];
#pragma unroll
    for (int i = 0; i < 50; ++i) q2[i] = ((const hvs_f2*)q)[i];
    float lds = 0.0f;
#pragma unroll 1
    for (uint32_t r = 0; r < 64u; ++r) {
        const uint32_t pr = p0 + r < last ? p0 + r : last;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        if (lane < 25u) srow[w][lane] = ((const float4*)(D + (size_t)pr * HVS_NDIM))[lane];
        if (lane == 25u) srow[w][25] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        const float v = hvs_exact_dist_pk_lds(srow[w], q2);
        if (lane == r) lds = v;
    }
    if (p0 + lane <= last) {
        o_plain[p] = hvs_make_key(plain, p);
        o_pk[p] = hvs_make_key(pk, p);
        o_lds[p] = hvs_make_key(lds, p);
        o_scalar[p] = hvs_make_key(scalar, p);
    }
}

// queries: [q0, q1, l, r] each; rows: [C, T] each.  params: [type, vf, l, r] as bits; pass: nq x nr
__global__ void hvp_k_pred(const float* __restrict__ Q, uint32_t nq, const float* __restrict__ rows, uint32_t nr, uint32_t* __restrict__ params,
                           uint32_t* __restrict__ pass)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const HvsQParams p = hvs_parse_query(Q + 4u * i);
    params[4u * i] = p.type;
    params[4u * i + 1u] = __float_as_uint(p.vf);
    params[4u * i + 2u] = __float_as_uint(p.l);
    params[4u * i + 3u] = __float_as_uint(p.r);
    for (uint32_t r = 0; r < nr; ++r) pass[(size_t)i * nr + r] = hvs_row_passes(p, rows[2u * r], rows[2u * r + 1u]) ? 1u : 0u;
}
__global__ void hvp_k_ordered(const float* __restrict__ f, uint32_t n, uint32_t* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = hvs_ordered_u32(f[i]);
}

// -------------------------------------------------------------------------------------------------------------- host side
typedef std::vector<uint32_t> Words;

static std::vector<Words> read_blobs(const char* path, int want)
{
    FILE* f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        exit(3);
    }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    Words all((size_t)bytes / 4u);
    if (fread(all.data(), 4, all.size(), f) != all.size() || all.size() < 2 || all[0] != HVP_MAGIC || (int)all[1] != want ||
        all.size() < 2u + 2u * (size_t)want) {
        fprintf(stderr, "%s: not a case file of %d blobs\n", path, want);
        exit(3);
    }
    fclose(f);
    std::vector<Words> blobs((size_t)want);
    for (int i = 0; i < want; ++i) {
        const size_t off = all[2 + 2 * i], len = all[3 + 2 * i];
        if (off + len > all.size()) {
            fprintf(stderr, "%s: blob %d outside the file\n", path, i);
            exit(3);
        }
        blobs[(size_t)i].assign(all.begin() + (long)off, all.begin() + (long)(off + len));
    }
    return blobs;
}

static void write_blobs(const char* path, const std::vector<Words>& blobs)
{
    Words head(2u + 2u * blobs.size());
    head[0] = HVP_MAGIC;
    head[1] = (uint32_t)blobs.size();
    size_t off = head.size() + (head.size() & 1u);
    for (size_t i = 0; i < blobs.size(); ++i) {
        head[2 + 2 * i] = (uint32_t)off;
        head[3 + 2 * i] = (uint32_t)blobs[i].size();
        off += blobs[i].size() + (blobs[i].size() & 1u);
    }
    FILE* f = fopen(path, "wb");
    if (!f) {
        fprintf(stderr, "cannot write %s\n", path);
        exit(3);
    }
    const uint32_t zero = 0u;
    fwrite(head.data(), 4, head.size(), f);
    if (head.size() & 1u) fwrite(&zero, 4, 1, f);
    for (const Words& b : blobs) {
        fwrite(b.data(), 4, b.size(), f);
        if (b.size() & 1u) fwrite(&zero, 4, 1, f);
    }
    if (fclose(f) != 0) {
        fprintf(stderr, "cannot write %s\n", path);
        exit(3);
    }
}

// a device copy of a blob (at least one word, so that no kernel is handed a null pointer); a few MB in all, released at exit
template <typename T>
static T* to_device(const Words& w)
{
    void* p = nullptr;
    CHECK(hipMalloc(&p, (w.size() + 2u) * 4u));
    CHECK(hipMemset(p, 0, (w.size() + 2u) * 4u));
    if (!w.empty()) CHECK(hipMemcpy(p, w.data(), w.size() * 4u, hipMemcpyHostToDevice));
    return (T*)p;
}
template <typename T>
static T* device_words(size_t words, int fill_byte)
{
    void* p = nullptr;
    CHECK(hipMalloc(&p, (words + 2u) * 4u));
    CHECK(hipMemset(p, fill_byte, (words + 2u) * 4u));
    return (T*)p;
}
static Words from_device(const void* p, size_t words)
{
    Words w(words);
    if (words) CHECK(hipMemcpy(w.data(), p, words * 4u, hipMemcpyDeviceToHost));
    return w;
}
static void finish(const char* section, uint32_t ncases, std::chrono::steady_clock::time_point t0)
{
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    printf("section %-10s cases %6u  %8.2f ms\n", section, ncases, ms);
    fflush(stdout);
}
static uint32_t grid4(uint32_t ncases) { return (ncases + 3u) / 4u; }

template <int NK, int FORM>
static void run_select(const Words& desc, const Words& lists, std::vector<Words>& out, int slot)
{
    constexpr size_t CAP = 64 * NK;
    const uint32_t n = (uint32_t)(desc.size() / 2u);
    if (lists.size() != (size_t)n * CAP * 2u) {
        fprintf(stderr, "select: %zu list words for %u cases\n", lists.size(), n);
        exit(3);
    }
    uint32_t* d_desc = to_device<uint32_t>(desc);
    uint64_t* d_in = to_device<uint64_t>(lists);
    uint64_t* d_out = to_device<uint64_t>(lists);
    uint64_t* d_kth = device_words<uint64_t>(2u * n, 0);
    if (n) hipLaunchKernelGGL((hvp_k_select<NK, FORM>), dim3(grid4(n)), dim3(256), 0, 0, d_desc, n, d_in, d_out, d_kth);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    out[(size_t)slot] = from_device(d_out, lists.size());
    out[(size_t)slot + 1u] = from_device(d_kth, 2u * n);
}

template <int CAP>
static void run_cut(const Words& desc, const Words& lists, std::vector<Words>& out, int slot)
{
    const uint32_t n = (uint32_t)(desc.size() / 4u);
    if (lists.size() != (size_t)n * CAP * 2u) exit(3);
    uint32_t* d_desc = to_device<uint32_t>(desc);
    uint64_t* d_in = to_device<uint64_t>(lists);
    uint64_t* d_out = device_words<uint64_t>(lists.size(), 0);
    uint32_t* d_ret = device_words<uint32_t>(n, 0xFF);
    uint64_t* d_kth = device_words<uint64_t>(2u * n, 0);
    if (n) hipLaunchKernelGGL((hvp_k_cut<CAP>), dim3(grid4(n)), dim3(256), 0, 0, d_desc, n, d_in, d_out, d_ret, d_kth);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    out[(size_t)slot] = from_device(d_out, lists.size());
    out[(size_t)slot + 1u] = from_device(d_ret, n);
    out[(size_t)slot + 2u] = from_device(d_kth, 2u * n);
}

template <int CAP>
static void run_gather(const Words& desc, const Words& lists, const uint32_t* d_ids, const float* d_dists, std::vector<Words>& out, int slot)
{
    const uint32_t n = (uint32_t)(desc.size() / 8u);
    if (lists.size() != (size_t)n * CAP * 2u) exit(3);
    uint32_t* d_desc = to_device<uint32_t>(desc);
    uint64_t* d_in = to_device<uint64_t>(lists);
    uint64_t* d_out = device_words<uint64_t>(lists.size(), 0);
    uint32_t* d_ret = device_words<uint32_t>(n, 0xFF);
    if (n) hipLaunchKernelGGL((hvp_k_gather<CAP>), dim3(grid4(n)), dim3(256), 0, 0, d_desc, n, d_in, d_ids, d_dists, d_out, d_ret);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    out[(size_t)slot] = from_device(d_out, lists.size());
    out[(size_t)slot + 1u] = from_device(d_ret, n);
}

template <int CAP>
static void run_dedup(const Words& desc, const Words& lists, std::vector<Words>& out, int slot)
{
    const uint32_t n = (uint32_t)(desc.size() / 2u);
    if (lists.size() != (size_t)n * CAP * 2u) exit(3);
    uint32_t* d_desc = to_device<uint32_t>(desc);
    uint64_t* d_in = to_device<uint64_t>(lists);
    uint64_t* d_out = device_words<uint64_t>(lists.size(), 0);
    uint32_t* d_ret = device_words<uint32_t>(n, 0xFF);
    if (n) hipLaunchKernelGGL((hvp_k_dedup<CAP>), dim3(grid4(n)), dim3(256), 0, 0, d_desc, n, d_in, d_out, d_ret);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    out[(size_t)slot] = from_device(d_out, lists.size());
    out[(size_t)slot + 1u] = from_device(d_ret, n);
}

int main(int argc, char** argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: %s CASES RESULTS\n", argv[0]);
        return 3;
    }
    const std::vector<Words> in = read_blobs(argv[1], IN_COUNT);
    std::vector<Words> out((size_t)OUT_COUNT);
    const auto t_all = std::chrono::steady_clock::now();
    CHECK(hipSetDevice(0));

    {  // ---- select
        const auto t0 = std::chrono::steady_clock::now();
        run_select<4, 0>(in[IN_SEL4_DESC], in[IN_SEL4_LISTS], out, OUT_SEL + 0);
        run_select<4, 1>(in[IN_SEL4_DESC], in[IN_SEL4_LISTS], out, OUT_SEL + 2);
        run_select<4, 2>(in[IN_SEL4_DESC], in[IN_SEL4_LISTS], out, OUT_SEL + 4);
        run_select<4, 3>(in[IN_SEL4_DESC], in[IN_SEL4_LISTS], out, OUT_SEL + 6);
        run_select<8, 0>(in[IN_SEL8_DESC], in[IN_SEL8_LISTS], out, OUT_SEL + 8);
        run_select<8, 1>(in[IN_SEL8_DESC], in[IN_SEL8_LISTS], out, OUT_SEL + 10);
        run_select<8, 2>(in[IN_SEL8_DESC], in[IN_SEL8_LISTS], out, OUT_SEL + 12);
        run_select<8, 3>(in[IN_SEL8_DESC], in[IN_SEL8_LISTS], out, OUT_SEL + 14);
        finish("select", (uint32_t)(in[IN_SEL4_DESC].size() / 2u + in[IN_SEL8_DESC].size() / 2u), t0);
    }
    {  // ---- make_room and final_cut
        const auto t0 = std::chrono::steady_clock::now();
        run_cut<256>(in[IN_CUT256_DESC], in[IN_CUT256_LISTS], out, OUT_CUT256_LISTS);
        run_cut<512>(in[IN_CUT512_DESC], in[IN_CUT512_LISTS], out, OUT_CUT512_LISTS);
        finish("cut", (uint32_t)(in[IN_CUT256_DESC].size() / 4u + in[IN_CUT512_DESC].size() / 4u), t0);
    }
    {  // ---- pad and rank
        const auto t0 = std::chrono::steady_clock::now();
        const uint32_t n = (uint32_t)(in[IN_PAD_DESC].size() / 8u);
        if (in[IN_PAD_LISTS].size() != (size_t)n * HVP_PAD_CAP * 2u) return 3;
        uint32_t* d_desc = to_device<uint32_t>(in[IN_PAD_DESC]);
        uint64_t* d_in = to_device<uint64_t>(in[IN_PAD_LISTS]);
        uint64_t* d_tab = to_device<uint64_t>(in[IN_PAD_TAB]);
        float* d_D = to_device<float>(in[IN_PAD_D]);
        float* d_Qx = to_device<float>(in[IN_PAD_QX]);
        uint64_t* d_out = device_words<uint64_t>(in[IN_PAD_LISTS].size(), 0);
        if (n) hipLaunchKernelGGL(hvp_k_pad, dim3(grid4(n)), dim3(256), 0, 0, d_desc, n, d_in, d_tab, d_D, d_Qx, d_out);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        out[OUT_PAD_LISTS] = from_device(d_out, in[IN_PAD_LISTS].size());

        const uint32_t nr = (uint32_t)(in[IN_RANK_DESC].size() / 4u);
        const size_t outlen = in[IN_RANK_OUTLEN].empty() ? 0u : in[IN_RANK_OUTLEN][0];
        uint32_t* r_desc = to_device<uint32_t>(in[IN_RANK_DESC]);
        uint64_t* r_keys = to_device<uint64_t>(in[IN_RANK_KEYS]);
        uint32_t* r_ids = device_words<uint32_t>(outlen, 0xEE);   // slots nothing writes keep 0xEEEEEEEE
        float* r_dists = device_words<float>(outlen, 0xEE);
        if (nr) hipLaunchKernelGGL(hvp_k_rank, dim3(grid4(nr)), dim3(256), 0, 0, r_desc, nr, r_keys, r_ids, r_dists);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        out[OUT_RANK_IDS] = from_device(r_ids, outlen);
        out[OUT_RANK_DISTS] = from_device(r_dists, outlen);
        finish("pad_rank", n + nr, t0);
    }
    {  // ---- keep, excluded, in_row_set
        const auto t0 = std::chrono::steady_clock::now();
        const uint32_t n = (uint32_t)(in[IN_KEEP_DESC].size() / 8u);
        if (in[IN_KEEP_LISTS].size() != (size_t)n * HVP_KEEP_CAP * 2u) return 3;
        const size_t ngroups = in[IN_KEEP_NGROUPS].empty() ? 0u : in[IN_KEEP_NGROUPS][0];
        uint32_t* d_desc = to_device<uint32_t>(in[IN_KEEP_DESC]);
        uint64_t* d_in = to_device<uint64_t>(in[IN_KEEP_LISTS]);
        uint32_t* d_cfg = to_device<uint32_t>(in[IN_EXCL_CFG]);
        uint32_t* d_pool = to_device<uint32_t>(in[IN_EXCL_POOL]);
        uint64_t* d_out = device_words<uint64_t>(in[IN_KEEP_LISTS].size(), 0);
        uint32_t* d_ret = device_words<uint32_t>(n, 0xFF);
        unsigned long long* d_ctr = device_words<unsigned long long>(ngroups * HVS_CNT_COUNT * 2u, 0);  // fresh and zeroed
        if (n) hipLaunchKernelGGL(hvp_k_keep, dim3(grid4(n)), dim3(256), 0, 0, d_desc, n, d_in, d_cfg, d_pool, d_out, d_ret, d_ctr);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        out[OUT_KEEP_LISTS] = from_device(d_out, in[IN_KEEP_LISTS].size());
        out[OUT_KEEP_RET] = from_device(d_ret, n);
        out[OUT_KEEP_COUNTERS] = from_device(d_ctr, ngroups * HVS_CNT_COUNT * 2u);

        const uint32_t ne = (uint32_t)(in[IN_EXQ_DESC].size() / 4u), ns = (uint32_t)(in[IN_SETQ_DESC].size() / 4u);
        uint32_t* e_desc = to_device<uint32_t>(in[IN_EXQ_DESC]);
        uint32_t* s_desc = to_device<uint32_t>(in[IN_SETQ_DESC]);
        uint32_t* e_out = device_words<uint32_t>(ne, 0xFF);
        uint32_t* s_out = device_words<uint32_t>(ns, 0xFF);
        if (ne) hipLaunchKernelGGL(hvp_k_excluded, dim3((ne + 255u) / 256u), dim3(256), 0, 0, e_desc, ne, d_pool, e_out);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        if (ns) hipLaunchKernelGGL(hvp_k_in_row_set, dim3((ns + 255u) / 256u), dim3(256), 0, 0, s_desc, ns, d_cfg, d_pool, s_out);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        out[OUT_EXQ] = from_device(e_out, ne);
        out[OUT_SETQ] = from_device(s_out, ns);
        finish("keep", n + ne + ns, t0);
    }
    {  // ---- gather
        const auto t0 = std::chrono::steady_clock::now();
        uint32_t* d_ids = to_device<uint32_t>(in[IN_GATH_IDS]);
        float* d_dists = to_device<float>(in[IN_GATH_DISTS]);
        run_gather<256>(in[IN_GATH256_DESC], in[IN_GATH256_LISTS], d_ids, d_dists, out, OUT_GATH256_LISTS);
        run_gather<512>(in[IN_GATH512_DESC], in[IN_GATH512_LISTS], d_ids, d_dists, out, OUT_GATH512_LISTS);
        finish("gather", (uint32_t)(in[IN_GATH256_DESC].size() / 8u + in[IN_GATH512_DESC].size() / 8u), t0);
    }
    {  // ---- dedup
        const auto t0 = std::chrono::steady_clock::now();
        run_dedup<256>(in[IN_DEDUP256_DESC], in[IN_DEDUP256_LISTS], out, OUT_DEDUP256_LISTS);
        run_dedup<512>(in[IN_DEDUP512_DESC], in[IN_DEDUP512_LISTS], out, OUT_DEDUP512_LISTS);
        finish("dedup", (uint32_t)(in[IN_DEDUP256_DESC].size() / 2u + in[IN_DEDUP512_DESC].size() / 2u), t0);
    }
    {  // ---- dist
        const auto t0 = std::chrono::steady_clock::now();
        const uint32_t np = (uint32_t)(in[IN_DIST_D].size() / HVS_NDIM);
        if (in[IN_DIST_Q].size() != in[IN_DIST_D].size()) return 3;
        float* d_D = to_device<float>(in[IN_DIST_D]);
        float* d_Q = to_device<float>(in[IN_DIST_Q]);
        uint64_t* o[4];
        for (int i = 0; i < 4; ++i) o[i] = device_words<uint64_t>(2u * np, 0xEE);
        if (np) hipLaunchKernelGGL(hvp_k_dist, dim3((np + 255u) / 256u), dim3(256), 0, 0, d_D, d_Q, np, o[0], o[1], o[2], o[3]);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        for (int i = 0; i < 4; ++i) out[(size_t)OUT_DIST_PLAIN + (size_t)i] = from_device(o[i], 2u * np);
        finish("dist", np, t0);
    }
    {  // ---- predicate
        const auto t0 = std::chrono::steady_clock::now();
        const uint32_t nq = (uint32_t)(in[IN_PRED_Q].size() / 4u), nr = (uint32_t)(in[IN_PRED_ROWS].size() / 2u);
        const uint32_t nf = (uint32_t)in[IN_ORD_F].size();
        float* d_Q = to_device<float>(in[IN_PRED_Q]);
        float* d_rows = to_device<float>(in[IN_PRED_ROWS]);
        float* d_f = to_device<float>(in[IN_ORD_F]);
        uint32_t* d_params = device_words<uint32_t>(4u * nq, 0xEE);
        uint32_t* d_pass = device_words<uint32_t>((size_t)nq * nr, 0xEE);
        uint32_t* d_ord = device_words<uint32_t>(nf, 0xEE);
        if (nq) hipLaunchKernelGGL(hvp_k_pred, dim3((nq + 255u) / 256u), dim3(256), 0, 0, d_Q, nq, d_rows, nr, d_params, d_pass);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        if (nf) hipLaunchKernelGGL(hvp_k_ordered, dim3((nf + 255u) / 256u), dim3(256), 0, 0, d_f, nf, d_ord);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        out[OUT_PRED_PARAMS] = from_device(d_params, 4u * nq);
        out[OUT_PRED_PASS] = from_device(d_pass, (size_t)nq * nr);
        out[OUT_ORD] = from_device(d_ord, nf);
        finish("predicate", nq + nf, t0);
    }
    write_blobs(argv[2], out);
    printf("total %.2f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_all).count());
    return 0;
}
