"""Cases and host models for tests/device_primitives.hip: the wave-level device primitives of csrc/hvs_device.h and
csrc/hvs_kernels.h, each run on its own (tests/test_primitives.py on the GPU, tests/test_primitives_cpu.py for the case set).

Plain numpy, seeded, nothing large committed.  The model of a select is a sort; the models of the other functions are their
documented contracts, quoted from the code comments:

* hvs_wave_select_prune: "Keys must be distinct ... `list` holds `cnt` keys ... Returns the KEEP-th smallest key; the list then
  holds exactly KEEP keys.  Precondition: cnt > KEEP" -- "an in-place ordered compaction"; "COMPACT = false: only the keep-th
  smallest key is returned, the list is left as it is".
* hvs_wave_make_room: "when they might not fit, the buffer is cut back to its knn smallest keys ... Returns the keys held; where
  it cut and `kth` is given, *kth is the largest key kept".  hvs_wave_final_cut: "the knn smallest of the keys held (distinct)
  stay.  Returns their number, <= knn".
* hvs_wave_pad: "Slot cnt + s takes key_of(s), s = 0 .. knn - cnt - 1 ... or with pad == 0 ... the largest key, which no row has".
* hvs_wave_rank_write: "Rank sort of exactly knn keys in the canonical order (dist ascending, id ascending; duplicates are
  possible after padding: ties broken by slot) ... ids, and distances where out_dists is not null (+inf for the key ~0)".
* hvs_keep_within: "those with `dist <= cap` are kept, packed in place in their order; returns their number ... (nor a NaN
  distance: `NaN <= cap` is false).  HVS_CNT_WITHIN_SLOTS += slots kept, HVS_CNT_WITHIN_UNDERFULL += 1 for an under-full query".
* hvs_keep_after: the test is `key >= lo`; "HVS_CNT_AFTER_SLOTS += slots kept, HVS_CNT_AFTER_UNDERFULL += 1 for an under-full
  query, HVS_CNT_AFTER_EXHAUSTED += 1 for an exhausted cursor" (lo == HVS_AFTER_NOTHING).
* hvs_keep_unlisted: keys of listed rows and of rows outside the query's set leave; "HVS_CNT_EXCL_SLOTS += slots kept,
  HVS_CNT_EXCL_UNDERFULL += 1 for an under-full query", and with set_of "the same two figures for hvs_row_sets_info" plus
  HVS_CNT_SET_RESTRICTED for "queries answered that carry a set index".
* hvs_excluded: "is `id` in the ascending list ids[0 .. count)?".  hvs_in_row_set: "set_of[q] is the set of resident query q ...
  or 0xFFFFFFFF for no restriction; nullptr while no query carries one.  Set s lies at set_bits[s * set_words ..), one bit per
  GLOBAL row (row i: bit i & 31 of word i >> 5), and the kernel's row ids start at global row `row0`".
* hvs_gather_list_keys: "One part's result row of one query -- `knn` slots, ids local to the part (0xFFFFFFFF = empty slot) --
  appended to the wave's key buffer as (dist bits << 32 | row0 + id) ... The buffer is cut back to its knn smallest keys
  whenever the next 64 slots might not fit".
* hvs_wave_dedup_ids: "de-duplicated BY ID, in place: per id the smallest key stays, and one of two equal keys ... The buffer is
  left in id order ... Returns the keys left".
* the distances: "8 strided accumulators, 12 full 8-wide steps over dims 0..95, masked tail adding dims 96..99 into accumulators
  4..7, reduction tree ((a0+a4)+(a1+a5)) + ((a2+a6)+(a3+a7)).  sub, mul, add are separate f32 roundings"; the sequential
  order "sum = sum + diff*diff for dims 0..99 in order"; hvs_make_key: "NaN (one canonical bit pattern) after +inf".
* hvs_parse_query: "query_type = uint32(q[0]); v = int32(q[1]) (truncation) ... t in (-1, 0) is type 0 ... Types outside 0..3
  (and values whose conversion is undefined behaviour in the reference) match no row: type 4".

Every expected output comes with a mask of the words the contract defines (a compaction says nothing about the words between
the keys it kept and the old end of the list); words behind `cnt` must always come back as they went in.  Every model takes a
set of WRONG RULES (RULES below): plausible mistakes of the function, as switches.  test_primitives_cpu.py shows that each
changes the expected output of some case, which is what makes the case set a test of that rule.
"""
import collections

import numpy as np

import hvs_testlib as T

MAGIC = 0x50535648
EMPTY = 0xFFFFFFFF
ALL1 = 0xFFFFFFFFFFFFFFFF
KTH_UNTOUCHED = 0x0DDBA11500C0FFEE
UNWRITTEN = 0xEEEEEEEE
INF_BITS, NAN_BITS = 0x7F800000, 0x7FC00000
CAP_NOTHING_BITS = 0xBF800000      # HVS_CAP_NOTHING = -1.0f
PAD_CAP, KEEP_CAP = 256, 512
CNT_COUNT = 38                     # HVS_CNT_COUNT and the slots the keep functions write (csrc/hvs_device.h)
CNT = dict(WITHIN_SLOTS=14, WITHIN_UNDERFULL=15, AFTER_SLOTS=16, AFTER_UNDERFULL=17, AFTER_EXHAUSTED=18, EXCL_SLOTS=20,
           EXCL_UNDERFULL=21, SET_SLOTS=30, SET_UNDERFULL=31, SET_RESTRICTED=33)

IN_BLOBS = ("SEL4_DESC SEL4_LISTS SEL8_DESC SEL8_LISTS CUT256_DESC CUT256_LISTS CUT512_DESC CUT512_LISTS "
            "PAD_DESC PAD_LISTS PAD_TAB PAD_D PAD_QX RANK_DESC RANK_KEYS RANK_OUTLEN "
            "KEEP_DESC KEEP_LISTS KEEP_NGROUPS EXCL_CFG EXCL_POOL EXQ_DESC SETQ_DESC "
            "GATH256_DESC GATH256_LISTS GATH512_DESC GATH512_LISTS GATH_IDS GATH_DISTS "
            "DEDUP256_DESC DEDUP256_LISTS DEDUP512_DESC DEDUP512_LISTS DIST_D DIST_Q PRED_Q PRED_ROWS ORD_F").split()
SELECT_FORMS = ("hist_compact", "hist_keep", "bits_lds", "bits_global")
OUT_BLOBS = (["SEL%d_%s_%s" % (nk, f, x) for nk in (4, 8) for f in SELECT_FORMS for x in ("LISTS", "KTH")] +
             "CUT256_LISTS CUT256_RET CUT256_KTH CUT512_LISTS CUT512_RET CUT512_KTH PAD_LISTS RANK_IDS RANK_DISTS "
             "KEEP_LISTS KEEP_RET KEEP_COUNTERS EXQ SETQ GATH256_LISTS GATH256_RET GATH512_LISTS GATH512_RET "
             "DEDUP256_LISTS DEDUP256_RET DEDUP512_LISTS DEDUP512_RET DIST_PLAIN DIST_PK DIST_LDS DIST_SCALAR "
             "PRED_PARAMS PRED_PASS ORD".split())
U64_OUT = {n for n in OUT_BLOBS if n.endswith(("_LISTS", "_KTH")) or n.startswith("DIST_") or n == "KEEP_COUNTERS"}

RULES = {
    "select": ("select_rank_plus_1", "select_compact_lt", "select_reads_past_cnt", "select_dist_only", "select_signed"),
    "pad_rank": ("rank_ties_unbroken", "rank_all1_as_nan", "pad_key_of_e", "pad0_pads_rows"),
    "keep": ("within_lt", "within_nan_passes", "after_gt", "exhausted_when_empty", "excluded_misses_first", "excluded_misses_last",
             "row_set_ignores_row0", "row_set_mirrored_bit"),
    "gather": ("gather_without_row0", "gather_reads_past_knn"),
    "dedup": ("dedup_keeps_largest", "dedup_keeps_both"),
    "dist": ("dist_fma", "dist_ftz", "dist_tail_into_0_3", "dist_seq_hsum", "dist_nan_raw"),
    "predicate": ("parse_v_rounded", "parse_type_floor"),
}
# "Ties by slot descending" in hvs_wave_rank_write is a switch too, but no case can tell it from the rule: two slots tie only
# when their keys are equal, and equal keys write the same id and the same distance whichever takes the lower rank.
# test_primitives_cpu.py asserts exactly that; the observable mistake next to it is rank_ties_unbroken (both take one rank).
UNOBSERVABLE_RULES = {"pad_rank": ("rank_ties_desc",)}

_u64 = np.uint64


def make_keys(bits, ids):
    return (np.asarray(bits, _u64) << _u64(32)) | np.asarray(ids, _u64)


def f32_bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def canon_bits(dist):
    """hvs_make_key's distance half: the float's bits, NaN as the one canonical pattern"""
    d = np.asarray(dist, np.float32)
    return np.where(np.isnan(d), np.uint32(NAN_BITS), d.view(np.uint32)).astype(np.uint32)


# ----------------------------------------------------------------------------------------------------------- blob files
def write_blobs(path, arrays):
    """[magic, n, (offset, length) x n, data]: u32 words, every blob 8-byte aligned"""
    words = [np.ascontiguousarray(a).view(np.uint32).ravel() for a in arrays]
    head = np.zeros(2 + 2 * len(words), np.uint32)
    head[0], head[1] = MAGIC, len(words)
    off = head.size + (head.size & 1)
    parts = [head] + ([np.zeros(1, np.uint32)] if head.size & 1 else [])
    for i, w in enumerate(words):
        head[2 + 2 * i], head[3 + 2 * i] = off, w.size
        parts.append(w)
        if w.size & 1:
            parts.append(np.zeros(1, np.uint32))
        off += w.size + (w.size & 1)
    np.concatenate(parts).tofile(path)


def read_blobs(path, names):
    raw = np.fromfile(path, np.uint32)
    assert raw[0] == MAGIC and raw[1] == len(names), "not a blob file of %d blobs" % len(names)
    out = {}
    for i, n in enumerate(names):
        off, ln = int(raw[2 + 2 * i]), int(raw[3 + 2 * i])
        w = raw[off:off + ln]
        out[n] = w.view(np.uint64) if n in U64_OUT else w
    return out


# ------------------------------------------------------------------------------------------------- the f32 distance model
def _ftz(x):
    x = np.asarray(x, np.float32)
    return np.where(np.abs(x) < np.float32(1.17549435e-38), np.float32(0) * x, x).astype(np.float32)


def _sq_add(acc, dv, qv, rules):
    """acc + (dv - qv)^2: three f32 roundings"""
    ftz = "dist_ftz" in rules
    t = (dv - qv).astype(np.float32)
    if ftz:
        t = _ftz(t)
    if "dist_fma" in rules:                    # the product unrounded: exact in f64 (24 x 24 bits)
        return (t.astype(np.float64) * t.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    t = (t * t).astype(np.float32)
    if ftz:
        t = _ftz(t)
    s = (acc + t).astype(np.float32)
    return _ftz(s) if ftz else s


def dist_simd_order(d, q, rules=frozenset()):
    """d, q: [n, 100] float32 -> [n] float32, the reference's SIMD order step by step"""
    d, q = np.asarray(d, np.float32), np.asarray(q, np.float32)
    with np.errstate(all="ignore"):
        acc = np.zeros((d.shape[0], 8), np.float32)
        for b in range(12):
            acc = _sq_add(acc, d[:, 8 * b:8 * b + 8], q[:, 8 * b:8 * b + 8], rules)
        lo = slice(0, 4) if "dist_tail_into_0_3" in rules else slice(4, 8)
        acc[:, lo] = _sq_add(acc[:, lo], d[:, 96:100], q[:, 96:100], rules)
        if "dist_seq_hsum" in rules:
            s = acc[:, 0]
            for j in range(1, 8):
                s = (s + acc[:, j]).astype(np.float32)
            return s
        s = (acc[:, 0:4] + acc[:, 4:8]).astype(np.float32)
        a, b2 = (s[:, 0] + s[:, 1]).astype(np.float32), (s[:, 2] + s[:, 3]).astype(np.float32)
        out = (a + b2).astype(np.float32)
        return _ftz(out) if "dist_ftz" in rules else out


def dist_scalar_order(d, q, rules=frozenset()):
    d, q = np.asarray(d, np.float32), np.asarray(q, np.float32)
    with np.errstate(all="ignore"):
        s = np.zeros(d.shape[0], np.float32)
        for i in range(100):
            s = _sq_add(s, d[:, i], q[:, i], rules)
        return s


def dist_keys(dist, rules=frozenset()):
    bits = f32_bits(dist) if "dist_nan_raw" in rules else canon_bits(dist)
    return make_keys(bits, np.arange(len(bits)))


class Section:
    """inputs: {blob name: array}; cases: {output blob name: [label per case]}; stride: {output blob name: words per case}"""

    def __init__(self, name):
        self.name, self.inputs, self.labels, self.stride = name, {}, {}, {}

    def expected(self, rules=frozenset()):      # -> {output blob name: (values, mask)}
        raise NotImplementedError


def _dirty_tail(keys, cap):
    """`cap` words: the keys, then words smaller than every key (0 where the smallest key leaves no room)"""
    keys = np.asarray(keys, _u64)
    out = np.zeros(cap, _u64)
    out[:keys.size] = keys
    lo = int(keys.min()) if keys.size else 1 << 40
    j = np.arange(cap - keys.size, dtype=np.int64)
    out[keys.size:] = [max(lo - 1 - int(x % 11), 0) for x in j]
    return out


def _distinct(rng, below, cnt):
    """cnt distinct integers in [0, below), in random order"""
    return rng.choice(below, cnt, replace=False).astype(np.uint64)


def _lists(case_keys, cap):
    return np.stack([_dirty_tail(k, cap) for k in case_keys]) if case_keys else np.zeros((0, cap), _u64)


# ------------------------------------------------------------------------------------------------------------- select
def _realistic_dists():
    D = T.gen_data_numpy(512)
    Q = T.gen_queries_numpy(4)
    return np.stack([dist_simd_order(D[:, 2:], np.repeat(Q[i:i + 1, 4:], 512, 0)) for i in range(4)])


def select_counts(nk):
    keeps = (8, 9, 63, 64, 65, 100, 128) if nk == 4 else (129, 200, 255, 256)
    cap = 64 * nk
    out = []
    for keep in keeps:
        for cnt in (keep + 1, keep + 2, 63, 64, 65, 127, 128, 129, cap - 1, cap):
            if keep < cnt <= cap and (cnt, keep) not in out:
                out.append((cnt, keep))
    return out


def _top_bit_keys(rng, t, cnt, keep):
    """cnt distinct keys that share every bit above t and differ in bit t, with x, x ^ 1 at ranks keep and keep + 1"""
    assert (2 << t) >= cnt
    while True:
        if t < 20:
            v = np.sort(rng.permutation(2 << t)[:cnt].astype(np.uint64))
        else:
            v = np.unique(rng.integers(0, 1 << 64, cnt + 8, dtype=np.uint64) >> _u64(63 - t))
            if v.size < cnt:
                continue
            v = np.sort(rng.permutation(v)[:cnt])
        x = v[keep - 1] & ~_u64(1)
        if keep >= 2 and v[keep - 2] == x:
            continue                                   # the pair would sit one rank early
        v[keep - 1], v[keep] = x, x | _u64(1)
        top = (v >> _u64(t)) & _u64(1)
        if top.min() == 0 and top.max() == 1 and np.unique(v).size == cnt:
            break
    prefix = (int(rng.integers(0, 1 << 62)) << (t + 1)) & ALL1 if t < 63 else 0
    return rng.permutation(v | _u64(prefix))


def _edge_keys(rng, kind, cnt, keep, t=44):
    """keys whose first digit (bits t-7 .. t) puts the keep-th key at a bucket edge"""
    lo = t - 7
    b = (3, 77, 200)
    if kind == "first":          # the first key of bucket 77
        c0 = keep - 1
        c1 = max(1, (cnt - c0) // 2)
    elif kind == "last":         # the last key of bucket 77
        c0, c1 = keep // 2, keep - keep // 2
    elif kind == "bucket0":
        b, c0, c1 = (0, 77, 200), (keep + 1 if cnt >= keep + 2 else keep), 0
    elif kind == "highest":      # the digit's last bucket
        b, c0, c1 = (3, 77, 255), 1, 1
    else:                        # "single": one key in the wanted bucket, rem == 1 on the first step
        c0, c1 = keep - 1, 1
    c = (c0, c1, cnt - c0 - c1)
    assert min(c) >= 0 and c[2] >= 1 and c[0] >= 1, (kind, cnt, keep, c)
    digs = np.repeat(np.array(b, np.uint64), c)
    low = _distinct(rng, 1 << 20, cnt) << _u64(lo - 20)      # distinct bits below the digit
    low |= rng.integers(0, 1 << (lo - 20), cnt).astype(np.uint64)
    prefix = _u64(0x3C << (t + 1))
    return rng.permutation(prefix | (digs << _u64(lo)) | low)


class Select(Section):
    def __init__(self, nk, seed=11):
        super().__init__("select")
        rng = np.random.default_rng(seed + nk)
        self.nk, self.cap = nk, 64 * nk
        counts = select_counts(nk)
        cases = []       # (family, params, keys, keep)
        tmin = 3 if nk == 4 else 7
        for t in range(tmin, 64):
            fit = [(c, k) for c, k in counts if (2 << t) >= c]
            for i in range(2):
                cnt, keep = fit[(t * 2 + i) % len(fit)]
                cases.append(("top_bit", "t=%d" % t, _top_bit_keys(rng, t, cnt, keep), keep))
        for kind in ("first", "last", "bucket0", "highest", "single"):
            for j, (cnt, keep) in enumerate(counts):
                if j % 3 == 0 or cnt == self.cap or cnt == keep + 1:
                    cases.append(("edge", kind, _edge_keys(rng, kind, cnt, keep, t=40 + j % 9), keep))
        real = _realistic_dists()
        for j, (cnt, keep) in enumerate(counts):
            bits = int(rng.integers(0x3F000000, 0x42000000))
            cases.append(("one_dist", "random ids", make_keys(np.full(cnt, bits), _distinct(rng, 1 << 24, cnt)), keep))
            cases.append(("one_dist", "consecutive ids", make_keys(np.full(cnt, bits), rng.permutation(cnt) + 1000 * j), keep))
            rows = rng.permutation(512)[:cnt]
            cases.append(("realistic", "query %d" % (j % 4), make_keys(canon_bits(real[j % 4][rows]), rows), keep))
            special = rng.choice(np.array([0, 0, INF_BITS, NAN_BITS, 0x3F800000, 0x00000001], np.uint64), cnt)
            ids = rng.permutation(4 * cnt)[:cnt].astype(np.uint64)
            k = make_keys(special, ids)
            if not (k == 0).any():
                k[int(rng.integers(cnt))] = 0                     # the key 0: distance +0 of row 0
            assert np.unique(k).size == cnt
            cases.append(("special", "0 inf nan", k, keep))
        self.cases = cases
        for f, p, k, keep in cases:
            assert np.unique(k).size == k.size and keep < k.size <= self.cap
        self.desc = np.array([[k.size, keep] for _, _, k, keep in cases], np.uint32)
        self.lists = _lists([k for _, _, k, _ in cases], self.cap)
        self.inputs = {"SEL%d_DESC" % nk: self.desc, "SEL%d_LISTS" % nk: self.lists}
        lab = ["%s %s cnt=%d keep=%d" % (f, p, k.size, keep) for f, p, k, keep in cases]
        for f in SELECT_FORMS:
            self.labels["SEL%d_%s_LISTS" % (nk, f)], self.stride["SEL%d_%s_LISTS" % (nk, f)] = lab, self.cap
            self.labels["SEL%d_%s_KTH" % (nk, f)], self.stride["SEL%d_%s_KTH" % (nk, f)] = lab, 1

    def expected(self, rules=frozenset()):
        n, cap = len(self.cases), self.cap
        kth = np.zeros(n, _u64)
        comp, cmask = self.lists.copy(), np.zeros((n, cap), bool)
        for i, (_, _, keys, keep) in enumerate(self.cases):
            cnt = keys.size
            pool = self.lists[i] if "select_reads_past_cnt" in rules else keys
            if "select_dist_only" in rules:
                order = np.argsort(pool >> _u64(32), kind="stable")
            elif "select_signed" in rules:
                order = np.argsort(pool.view(np.int64), kind="stable")
            else:
                order = np.argsort(pool, kind="stable")           # the model of a select is a sort
            kk = pool[order[keep if "select_rank_plus_1" in rules else keep - 1]]
            kth[i] = kk
            if "select_dist_only" in rules:
                kept = pool[(pool >> _u64(32)) <= (kk >> _u64(32))]
            elif "select_signed" in rules:
                kept = pool[pool.view(np.int64) <= np.int64(np.uint64(kk).view(np.int64))]
            elif "select_compact_lt" in rules:
                kept = pool[pool < kk]
            else:
                kept = pool[pool <= kk]
            m = min(kept.size, cap)
            comp[i, :m] = kept[:m]
            cmask[i, :max(m, keep)] = True
            cmask[i, cnt:] = True                                 # behind cnt: as it went in
        full = np.ones((n, cap), bool)
        out = {}
        for f in SELECT_FORMS:
            nm = "SEL%d_%s_" % (self.nk, f)
            out[nm + "KTH"] = (kth, np.ones(n, bool))
            out[nm + "LISTS"] = (self.lists.ravel(), full.ravel()) if f == "hist_keep" else (comp.ravel(), cmask.ravel())
        return out

    def trace(self, i):
        """The histogram descent's control flow on case i, for coverage conditions only: per step the digit's width, whether
        the rank fell on its bucket's first / last key, the bucket's size and place."""
        _, _, keys, keep = self.cases[i]
        ks = [int(k) for k in keys]
        d = 0
        for k in ks:
            d |= k ^ ks[0]
        hi = d.bit_length() - 1 if d else 0
        r, steps = keep, []
        while True:
            lo = max(hi - 7, 0)
            width = hi - lo + 1
            cnts = collections.Counter((k >> lo) & ((1 << width) - 1) for k in ks)
            before = 0
            for dg in sorted(cnts):
                if before < r <= before + cnts[dg]:
                    break
                before += cnts[dg]
            steps.append(dict(width=width, lo=lo, hi=hi, first=r == before + 1, last=r == before + cnts[dg], rem=cnts[dg],
                              bucket0=dg == 0, top_bucket=dg == (1 << width) - 1))
            r -= before
            ks = [k for k in ks if (k >> lo) & ((1 << width) - 1) == dg]
            if cnts[dg] == 1 or lo == 0:
                return steps
            hi = lo - 1


# ----------------------------------------------------------------------------------------------- make_room and final_cut
def _random_keys(rng, cnt, id_lo=0, id_hi=1 << 24):
    bits = rng.integers(0x41000000, 0x41000400, cnt).astype(np.uint64)        # a narrow band: many equal distances
    return make_keys(bits, _distinct(rng, id_hi - id_lo, cnt) + _u64(id_lo))


class Cut(Section):
    def __init__(self, cap, seed=23):
        super().__init__("cut")
        rng = np.random.default_rng(seed + cap)
        self.cap = cap
        rows = []    # (cnt, step, knn, op)
        for knn in ((8, 100, 128) if cap == 256 else (129, 200, 256)):
            for op in (0, 1):
                for cnt, step in ((cap - 64, 64), (cap - 63, 64), (cap, 64), (knn + 1, cap - knn), (knn + 1, cap - knn - 1), (0, 64),
                                  (knn, 64), (cap - 1, 1), (cap, 1), (cap - 1, 2)):
                    if knn + step <= cap and (cnt + step <= cap or cnt > knn):
                        rows.append((cnt, step, knn, op))
            for cnt in (0, 1, knn - 1, knn, knn + 1, knn + 2, cap - 1, cap):
                rows.append((cnt, 0, knn, 2))
        self.rows = rows
        self.keys = [_random_keys(rng, r[0]) for r in rows]
        self.lists = _lists(self.keys, cap)
        self.inputs = {"CUT%d_DESC" % cap: np.array(rows, np.uint32), "CUT%d_LISTS" % cap: self.lists}
        lab = ["%s cnt=%d step=%d knn=%d" % (("make_room+kth", "make_room", "final_cut")[op], c, s, k) for c, s, k, op in rows]
        for x, st in (("LISTS", cap), ("RET", 1), ("KTH", 1)):
            self.labels["CUT%d_%s" % (cap, x)], self.stride["CUT%d_%s" % (cap, x)] = lab, st

    def expected(self, rules=frozenset()):
        n, cap = len(self.rows), self.cap
        lists, mask = self.lists.copy(), np.ones((n, cap), bool)
        ret, kth = np.zeros(n, np.uint32), np.full(n, KTH_UNTOUCHED, _u64)
        for i, ((cnt, step, knn, op), keys) in enumerate(zip(self.rows, self.keys)):
            cut = cnt > knn if op == 2 else cnt + step > cap
            ret[i] = knn if cut else cnt
            if cut:
                kk = np.sort(keys)[knn - 1]
                lists[i, :knn] = keys[keys <= kk]
                mask[i, knn:cnt] = False
                if op == 0:
                    kth[i] = kk
        nm = "CUT%d_" % cap
        return {nm + "LISTS": (lists.ravel(), mask.ravel()), nm + "RET": (ret, np.ones(n, bool)), nm + "KTH": (kth, np.ones(n, bool))}


# --------------------------------------------------------------------------------------------------------- pad and rank
class PadRank(Section):
    N_ROWS, N_Q = 300, 6

    def __init__(self, seed=31):
        super().__init__("pad_rank")
        rng = np.random.default_rng(seed)
        self._keys = None
        self.D = T.gen_data_numpy(self.N_ROWS, seed=77)
        self.Qx = T.gen_queries_numpy(self.N_Q, seed=78)
        self.Qx[4, 4:] = np.float32(3e19)                          # a query vector whose every distance overflows: +inf keys
        rows, tabs, tab_off = [], [], 0
        for knn in (256, 100, 65, 8):
            for diff in sorted({0, 1, 63, 64, 65, 200, knn}):
                if diff > knn:
                    continue
                for pad in (0, 1):
                    modes = [(0, 0, 0)]
                    if diff in (1, 65, knn):
                        modes += [(1, 1, 0), (2, 2, 0), (3, 1, 4), (4, 0, 3), (3, 3, 3), (1, 4, 0), (3, 3, 6)]
                    for mode, qa, qb in modes:
                        rows.append([knn - diff, knn, pad, mode, tab_off, qa, qb, self.N_ROWS])
                        tabs.append(_random_keys(rng, knn))        # knn entries: only the first knn - cnt are the rule's
                        tab_off += knn
        self.rows = rows
        self.tab = np.concatenate(tabs)
        self.lists = np.stack([rng.integers(0, 1 << 63, PAD_CAP).astype(np.uint64) for _ in rows])
        # rank: exactly knn keys per case; result row `row` of knn slots, rows chosen so that no two cases overlap
        rk, keys, off, end = [], [], 0, 0
        for knn in (8, 37, 64, 65, 100, 256):
            base = _random_keys(rng, knn)
            runs = base.copy()
            runs[rng.integers(0, knn, knn)] = runs[rng.integers(0, knn, knn)]      # runs of duplicate keys
            empt = base.copy()
            empt[rng.permutation(knn)[:max(3, knn // 5)]] = ALL1                    # several ~0
            nonf = base.copy()
            sel = rng.permutation(knn)[:max(4, knn // 4)]
            nonf[sel] = make_keys(rng.choice(np.array([INF_BITS, NAN_BITS], np.uint64), sel.size), nonf[sel] & _u64(EMPTY))
            padded = np.concatenate([base[:knn // 2], np.repeat(base[knn // 2:knn // 2 + 1], knn - knn // 2)])
            for fam, k in (("distinct", base), ("duplicate runs", runs), ("several ~0", empt), ("nan inf", nonf), ("one pad row", padded)):
                for with_d in (1, 0):
                    row = -(-end // knn)
                    rk.append((knn, with_d, row, off, fam))
                    keys.append(k)
                    off += knn
                    end = (row + 1) * knn
        self.rk, self.rkeys, self.rank_len = rk, keys, end
        self.inputs = {"PAD_DESC": np.array(rows, np.uint32), "PAD_LISTS": self.lists, "PAD_TAB": self.tab, "PAD_D": self.D,
                       "PAD_QX": self.Qx, "RANK_DESC": np.array([r[:4] for r in rk], np.uint32), "RANK_KEYS": np.concatenate(keys),
                       "RANK_OUTLEN": np.array([end], np.uint32)}
        self.labels["PAD_LISTS"] = ["pad cnt=%d knn=%d pad=%d mode=%d q=[%d,%d)" % (r[0], r[1], r[2], r[3], r[5], r[6]) for r in rows]
        self.stride["PAD_LISTS"] = PAD_CAP
        self.slot_case = np.full(end, -1)
        for i, (knn, _, row, _, _) in enumerate(rk):
            self.slot_case[row * knn:(row + 1) * knn] = i
        rl = ["rank %s knn=%d dists=%d" % (r[4], r[0], r[1]) for r in rk]
        self.labels["RANK_IDS"] = self.labels["RANK_DISTS"] = rl

    def _row_key(self, scalar, rid, qrows):
        """hvs_row_key / hvs_row_key_min of row `rid` over the query rows `qrows` (none: the key ~0)"""
        if self._keys is None:      # [order][query row][row of D]
            rid_all = np.arange(self.N_ROWS)
            self._keys = [[make_keys(canon_bits(fn(self.D[:, 2:], np.repeat(self.Qx[j:j + 1, 4:], self.N_ROWS, 0))), rid_all)
                           for j in range(self.N_Q)] for fn in (dist_simd_order, dist_scalar_order)]
        return min([int(self._keys[int(scalar)][j][rid]) for j in qrows], default=ALL1)

    def expected(self, rules=frozenset()):
        lists = self.lists.copy()
        for i, (cnt, knn, pad, mode, toff, qa, qb, n) in enumerate(self.rows):
            for e in range(cnt, knn):
                s = e if "pad_key_of_e" in rules else e - cnt
                if not pad and "pad0_pads_rows" not in rules:
                    lists[i, e] = ALL1
                elif mode == 0:
                    lists[i, e] = self.tab[toff + s]
                else:
                    lists[i, e] = self._row_key(mode in (2, 4), n - 1 - s, [qa] if mode < 3 else range(qa, qb))
        ids = np.full(self.rank_len, UNWRITTEN, np.uint32)
        dists = np.full(self.rank_len, UNWRITTEN, np.uint32)
        for (knn, with_d, row, _, _), k in zip(self.rk, self.rkeys):
            order = np.argsort(k, kind="stable")                   # dist, id, then slot
            if "rank_ties_desc" in rules:
                order = np.lexsort((-np.arange(knn), k))
            o = slice(row * knn, (row + 1) * knn)
            sk = k[order]
            if "rank_ties_unbroken" in rules:                      # equal keys share the lowest rank of their run
                first = np.searchsorted(sk, sk, "left")
                keep = np.zeros(knn, bool)
                keep[first] = True
            else:
                keep = np.ones(knn, bool)
            ids[o] = np.where(keep, (sk & _u64(EMPTY)).astype(np.uint32), np.uint32(UNWRITTEN))
            if with_d:
                db = (sk >> _u64(32)).astype(np.uint32)
                if "rank_all1_as_nan" not in rules:
                    db = np.where(sk == _u64(ALL1), np.uint32(INF_BITS), db)
                dists[o] = np.where(keep, db, np.uint32(UNWRITTEN))
        full = np.ones(self.rank_len, bool)
        return {"PAD_LISTS": (lists.ravel(), np.ones(lists.size, bool)), "RANK_IDS": (ids, full), "RANK_DISTS": (dists, full)}


# ----------------------------------------------------------------------------------------------------------------- keep
LIST_LENS = (0, 1, 2, 3, 64, 1023, 1024)
SET_WORDS, N_SETS = 80, 3


def excluded(lst, ids, rules=frozenset()):
    """hvs_excluded for an array of ids"""
    if "excluded_misses_first" in rules:
        lst = lst[1:]
    if "excluded_misses_last" in rules:
        lst = lst[:-1]
    return np.isin(np.asarray(ids, np.int64), lst.astype(np.int64))


def in_row_set(cfg, qi, ids, rules=frozenset()):
    """hvs_in_row_set for an array of ids.  cfg: dict(set_of, set_bits, row0) -- set_of None for nullptr"""
    ids = np.asarray(ids, np.int64)
    if cfg["set_of"] is None or cfg["set_of"][qi] == EMPTY:
        return np.ones(ids.shape, bool)
    g = ids + (0 if "row_set_ignores_row0" in rules else cfg["row0"])
    bit = 31 - (g & 31) if "row_set_mirrored_bit" in rules else g & 31
    words = cfg["set_bits"][int(cfg["set_of"][qi]) * SET_WORDS + (g >> 5)].astype(np.int64)
    return ((words >> bit) & 1) != 0


class Keep(Section):
    def __init__(self, seed=41):
        super().__init__("keep")
        rng = np.random.default_rng(seed)
        # the pool: lists (ascending, a gap after every entry), begin / count, three set_of tables, the sets' bits
        self.lists_ids = [np.array([5 + 2 * i for i in range(n)], np.uint32) for n in LIST_LENS]
        nq = len(LIST_LENS)
        pool, at = [], {}

        def put(name, a):
            at[name] = sum(p.size for p in pool)
            pool.append(np.asarray(a, np.uint32))
        ids_all = np.concatenate(self.lists_ids)
        begin = np.cumsum([0] + [x.size for x in self.lists_ids[:-1]])
        put("ids", ids_all)
        put("begin", begin)
        put("count", [x.size for x in self.lists_ids])
        self.set_of = [None, np.array([EMPTY, 0, 1, 2, EMPTY, 1, 2], np.uint32), np.array([2, EMPTY, 0, 1, 2, 2, 0], np.uint32)]
        put("set_of1", self.set_of[1])
        put("set_of2", self.set_of[2])
        self.set_bits = rng.integers(0, 1 << 32, N_SETS * SET_WORDS, dtype=np.uint64).astype(np.uint32)
        put("set_bits", self.set_bits)
        self.pool, self.at = np.concatenate(pool), at
        self.begin = begin
        row0s = (0, 0, 37)
        self.cfgs = [dict(set_of=self.set_of[c], set_bits=self.set_bits, row0=row0s[c]) for c in range(3)]
        cfg_words = [[at["begin"], at["count"], at["ids"], EMPTY if c == 0 else at["set_of%d" % c], at["set_bits"], SET_WORDS, row0s[c], 0]
                     for c in range(3)]
        max_id = SET_WORDS * 32 - 37
        assert int(ids_all.max()) + 2 < max_id
        rows, keys, lab = [], [], []     # desc rows [fn, cnt, knn, count, group, p0, p1, 0]
        dist_pool = np.array([0, 0x3F800000, 0x3F800001, 0x40000000, 0x7F7FFFFF, INF_BITS, NAN_BITS], np.uint64)
        group = 0
        for count in (1, 0):
            for cnt in (1, 64, 65, 256, 512):
                k = make_keys(rng.choice(dist_pool, cnt), _distinct(rng, 1 << 20, cnt))
                if cnt >= 64:
                    k[:7] = make_keys(dist_pool, k[:7] & _u64(EMPTY))          # every distance present
                    k = rng.permutation(k)
                caps = (("inf", INF_BITS), ("nothing", CAP_NOTHING_BITS), ("zero", 0), ("a key's", 0x3F800001), ("below it", 0x3F800000),
                        ("max", 0x7F7FFFFF), ("below 1", 0x3F7FFFFF))
                for j, (nm, cap) in enumerate(caps):
                    rows.append([0, cnt, (1, cnt, 100)[j % 3], count, group, cap, 0, 0])
                    keys.append(k)
                    lab.append("keep_within cap=%s cnt=%d count=%d" % (nm, cnt, count))
            group += 1
            for cnt in (1, 64, 65, 256, 512):
                k = make_keys(rng.choice(dist_pool[:5], cnt), _distinct(rng, 1 << 20, cnt))
                plain = k.copy()
                if cnt > 1:
                    k[0] = ALL1                                                 # an empty-slot key: >= every cursor, ~0 included
                    k = rng.permutation(k)
                present = int(np.sort(plain)[cnt // 2])
                for j, (nm, lo) in enumerate((("0", 0), ("present", present), ("present+1", present + 1), ("nothing", ALL1),
                                              ("behind all", int(plain.max()) + 1))):
                    kk = plain if nm in ("behind all", "present", "present+1") else k
                    rows.append([1, cnt, (1, cnt, 100)[j % 3], count, group, lo & EMPTY, lo >> 32, 0])
                    keys.append(kk)
                    lab.append("keep_after lo=%s cnt=%d count=%d" % (nm, cnt, count))
            group += 1
            for cfg in range(3):
                for qi, lst in enumerate(self.lists_ids):
                    # ids: the entries, every gap, below the first, above the last, word edges of the set
                    edges = [g - row0s[cfg] for g in (31, 32, 63, 64, 95, 96) if g >= row0s[cfg]]
                    cand = np.concatenate([lst, lst + 1, [4, 3, 0, int(lst.max()) + 2 if lst.size else 9], edges,
                                           rng.integers(0, max_id, 600)]).astype(np.int64)       # ... and rows anywhere in the sets' window
                    cand = rng.permutation(np.unique(cand[cand < max_id]))
                    must = list(dict.fromkeys([int(lst[0]), int(lst[-1])])) if lst.size else []      # the first and the last entry, always
                    order = must + [int(x) for x in cand if int(x) not in must]
                    for cnt in (1, 64, 65, 256, 512):
                        if cnt > len(order):
                            continue
                        ids = np.array(order[:cnt], np.uint64)
                        rows.append([2, ids.size, (1, ids.size, 100)[(qi + cnt) % 3], count, group, cfg, qi, 0])
                        keys.append(make_keys(rng.choice(dist_pool[:5], ids.size), ids))
                        lab.append("keep_unlisted cfg=%d list_len=%d cnt=%d count=%d" % (cfg, lst.size, ids.size, count))
                group += 1
        self.rows, self.keys, self.ngroups = rows, keys, group
        self.lists = _lists(keys, KEEP_CAP)
        # the admission tests on their own: every entry, every gap, both ends; every row of the sets' window
        exq = []
        for qi, lst in enumerate(self.lists_ids):
            for rid in np.unique(np.concatenate([lst, lst + 1, [4, 0, EMPTY]])):
                exq.append([at["ids"] + int(begin[qi]), lst.size, int(rid), qi])
        self.exq = exq
        setq = []
        for cfg in range(3):
            for qi in range(nq):
                for rid in list(range(0, 130)) + [max_id - 1]:
                    setq.append([cfg, qi, rid, 0])
        self.setq = setq
        self.inputs = {"KEEP_DESC": np.array(rows, np.uint32), "KEEP_LISTS": self.lists, "KEEP_NGROUPS": np.array([group], np.uint32),
                       "EXCL_CFG": np.array(cfg_words, np.uint32), "EXCL_POOL": self.pool, "EXQ_DESC": np.array(exq, np.uint32),
                       "SETQ_DESC": np.array(setq, np.uint32)}
        self.labels = {"KEEP_LISTS": lab, "KEEP_RET": lab, "EXQ": ["hvs_excluded list_len=%d id=%d" % (e[1], e[2]) for e in exq],
                       "SETQ": ["hvs_in_row_set cfg=%d q=%d id=%d" % (s[0], s[1], s[2]) for s in setq],
                       "KEEP_COUNTERS": ["counter group %d slot %d" % (g, s) for g in range(group) for s in range(CNT_COUNT)]}
        self.stride = {"KEEP_LISTS": KEEP_CAP, "KEEP_RET": 1, "EXQ": 1, "SETQ": 1, "KEEP_COUNTERS": 1}

    def expected(self, rules=frozenset()):
        n = len(self.rows)
        lists, mask = self.lists.copy(), np.ones((n, KEEP_CAP), bool)
        ret = np.zeros(n, np.uint32)
        ctr = np.zeros((self.ngroups, CNT_COUNT), _u64)
        for i, ((fn, cnt, knn, count, group, p0, p1, _), k) in enumerate(zip(self.rows, self.keys)):
            c = ctr[group]
            if fn == 0:
                d = (k >> _u64(32)).astype(np.uint32).view(np.float32)
                cap = np.array([p0], np.uint32).view(np.float32)[0]
                with np.errstate(invalid="ignore"):
                    keep = d < cap if "within_lt" in rules else ~(d > cap) if "within_nan_passes" in rules else d <= cap
                names = ("WITHIN_SLOTS", "WITHIN_UNDERFULL")
            elif fn == 1:
                lo = _u64(p0 | (p1 << 32))
                keep = k > lo if "after_gt" in rules else k >= lo
                names = ("AFTER_SLOTS", "AFTER_UNDERFULL")
            else:
                cfg, lst = self.cfgs[p0], self.lists_ids[p1]
                rid = (k & _u64(EMPTY)).astype(np.int64)
                keep = ~excluded(lst, rid, rules) & in_row_set(cfg, p1, rid, rules)
                names = ("EXCL_SLOTS", "EXCL_UNDERFULL")
            kept = int(keep.sum())
            lists[i, :kept] = k[keep]
            mask[i, kept:cnt] = False
            ret[i] = kept
            if count:
                c[CNT[names[0]]] += kept
                c[CNT[names[1]]] += kept < knn
                if fn == 1:
                    c[CNT["AFTER_EXHAUSTED"]] += kept == 0 if "exhausted_when_empty" in rules else int(lo) == ALL1
                if fn == 2 and cfg["set_of"] is not None:
                    c[CNT["SET_SLOTS"]] += kept
                    c[CNT["SET_UNDERFULL"]] += kept < knn
                    c[CNT["SET_RESTRICTED"]] += cfg["set_of"][p1] != EMPTY
        exq = np.array([excluded(self.lists_ids[qi], [rid], rules)[0] for _, _, rid, qi in self.exq], np.uint32)
        setq = np.array([in_row_set(self.cfgs[c], qi, [rid], rules)[0] for c, qi, rid, _ in self.setq], np.uint32)
        one = lambda a: (a, np.ones(a.size, bool))
        return {"KEEP_LISTS": (lists.ravel(), mask.ravel()), "KEEP_RET": one(ret), "KEEP_COUNTERS": one(ctr.ravel()), "EXQ": one(exq),
                "SETQ": one(setq)}


# --------------------------------------------------------------------------------------------------------------- gather
class Gather(Section):
    def __init__(self, seed=53):
        super().__init__("gather")
        rng = np.random.default_rng(seed)
        self.by_cap = {256: [], 512: []}
        ids_pool, dist_pool, off = [], [], 0
        for cap, knns in ((256, (8, 64, 65, 100)), (512, (100, 256))):
            for knn in knns:
                for cnt0 in sorted({0, 5, knn, cap - 64, cap - 63, cap - 64 - knn // 2, cap}):
                    if cnt0 < 0:
                        continue
                    for fill in ("full", "interleaved", "empty"):
                        for row0 in (0, 0x1FFFFF000, 0xFFFFFFF0):
                            ids = (rng.permutation(1 << 12)[:knn + 64] + 16).astype(np.uint32)    # + 64 behind slot knn - 1, all real
                            if fill == "interleaved":
                                ids[:knn][rng.random(knn) < 0.4] = EMPTY
                                ids[0] = EMPTY                                  # an empty slot that is not at the end
                            if fill == "empty":
                                ids[:knn] = EMPTY
                            d = rng.integers(0x41000000, 0x41000400, knn + 64).astype(np.uint32)
                            d[knn:] = 0x3F000000                                # smaller than every real key: they would stay
                            d[rng.integers(knn)] = 0x7FA00001                   # a NaN that is not the canonical one
                            d[rng.integers(knn)] = INF_BITS
                            buf = _random_keys(rng, cnt0, 1 << 22, 1 << 23)    # ids no gathered key has
                            self.by_cap[cap].append(dict(cnt0=cnt0, knn=knn, ids=ids, dists=d, row0=row0, off=off, buf=buf, fill=fill))
                            ids_pool.append(ids)
                            dist_pool.append(d)
                            off += knn + 64
        self.inputs = {"GATH_IDS": np.concatenate(ids_pool), "GATH_DISTS": np.concatenate(dist_pool)}
        for cap, cs in self.by_cap.items():
            self.inputs["GATH%d_DESC" % cap] = np.array([[c["cnt0"], c["knn"], c["off"], c["off"], c["row0"] & EMPTY, c["row0"] >> 32, 0, 0]
                                                         for c in cs], np.uint32)
            self.inputs["GATH%d_LISTS" % cap] = _lists([c["buf"] for c in cs], cap)
            lab = ["gather CAP=%d knn=%d cnt0=%d %s row0=%#x" % (cap, c["knn"], c["cnt0"], c["fill"], c["row0"]) for c in cs]
            self.labels["GATH%d_LISTS" % cap] = self.labels["GATH%d_RET" % cap] = lab
            self.stride["GATH%d_LISTS" % cap], self.stride["GATH%d_RET" % cap] = cap, 1

    def expected(self, rules=frozenset()):
        out = {}
        for cap, cs in self.by_cap.items():
            lists, mask = np.zeros((len(cs), cap), _u64), np.zeros((len(cs), cap), bool)
            ret = np.zeros(len(cs), np.uint32)
            for i, c in enumerate(cs):
                buf, knn = [int(x) for x in c["buf"]], c["knn"]
                row0 = 0 if "gather_without_row0" in rules else c["row0"]
                bits = canon_bits(c["dists"].view(np.float32))
                for o in range(0, knn, 64):
                    if len(buf) + 64 > cap:
                        kk = sorted(buf)[knn - 1]
                        buf = [x for x in buf if x <= kk]
                    end = o + 64 if "gather_reads_past_knn" in rules else min(o + 64, knn)
                    buf += [(int(bits[e]) << 32) | ((row0 + int(c["ids"][e])) & EMPTY) for e in range(o, end) if c["ids"][e] != EMPTY]
                ret[i] = len(buf)
                m = min(len(buf), cap)
                lists[i, :m], mask[i, :m] = buf[:m], True
            out["GATH%d_LISTS" % cap] = (lists.ravel(), mask.ravel())
            out["GATH%d_RET" % cap] = (ret, np.ones(len(cs), bool))
        return out


# ---------------------------------------------------------------------------------------------------------------- dedup
class Dedup(Section):
    def __init__(self, seed=61):
        super().__init__("dedup")
        rng = np.random.default_rng(seed)
        self.by_cap = {}
        for cap in (256, 512):
            cs = []
            for cnt in (0, 1, 2, 63, 64, 65, 128, 129, 256, 512):
                if cnt > cap:
                    continue
                for fam in ("no duplicates", "runs", "exact duplicates", "one id"):
                    bits = rng.integers(0x41000000, 0x41000040, cnt).astype(np.uint64)
                    ids = rng.permutation(1 << 16)[:cnt].astype(np.uint64)
                    if fam == "runs" and cnt:                                   # runs of 2 .. 64 keys of one id
                        runs = []
                        while sum(runs) < cnt:
                            runs.append(int(rng.integers(2, 65)))
                        ids = np.repeat(ids[:len(runs)], runs)[:cnt]
                    if fam == "one id":
                        ids[:] = 4242
                    k = make_keys(bits, ids)
                    if fam == "exact duplicates" and cnt > 1:
                        k[rng.integers(0, cnt, cnt // 2 + 1)] = k[rng.integers(0, cnt, cnt // 2 + 1)]
                    cs.append((fam, rng.permutation(k)))
            self.by_cap[cap] = cs
            self.inputs["DEDUP%d_DESC" % cap] = np.array([[k.size, 0] for _, k in cs], np.uint32)
            self.inputs["DEDUP%d_LISTS" % cap] = _lists([k for _, k in cs], cap)
            lab = ["dedup CAP=%d %s cnt=%d" % (cap, f, k.size) for f, k in cs]
            self.labels["DEDUP%d_LISTS" % cap] = self.labels["DEDUP%d_RET" % cap] = lab
            self.stride["DEDUP%d_LISTS" % cap], self.stride["DEDUP%d_RET" % cap] = cap, 1

    def expected(self, rules=frozenset()):
        out = {}
        for cap, cs in self.by_cap.items():
            lists, mask = np.zeros((len(cs), cap), _u64), np.zeros((len(cs), cap), bool)
            ret = np.zeros(len(cs), np.uint32)
            for i, (_, k) in enumerate(cs):
                best = {}
                for x in (int(v) for v in k):
                    rid = x & EMPTY
                    if "dedup_keeps_both" in rules:
                        best.setdefault(rid, []).append(x)
                    elif rid not in best or (x > best[rid][0] if "dedup_keeps_largest" in rules else x < best[rid][0]):
                        best[rid] = [x]
                if "dedup_keeps_both" in rules:                                 # equal keys both stay; of different keys the smallest
                    best = {r: [x for x in v if x == min(v)] for r, v in best.items()}
                res = [x for r in sorted(best) for x in best[r]]
                ret[i] = len(res)
                lists[i, :len(res)], mask[i, :len(res)] = res, True
            out["DEDUP%d_LISTS" % cap] = (lists.ravel(), mask.ravel())
            out["DEDUP%d_RET" % cap] = (ret, np.ones(len(cs), bool))
        return out


# ----------------------------------------------------------------------------------------------------------------- dist
DIST_FAMILIES = ("uniform", "wide", "tiny", "edge_of_normal", "overflow", "near_overflow", "non_finite", "known_answer")
PAIRS = 256


def dist_family(name, seed=71):
    rng = np.random.default_rng(seed + DIST_FAMILIES.index(name))
    n = PAIRS
    if name == "uniform":
        return rng.uniform(-6, 6, (n, 100)).astype(np.float32), rng.uniform(-6, 6, (n, 100)).astype(np.float32)
    if name == "wide":
        g = lambda: (np.sign(rng.standard_normal((n, 100))) * 10.0 ** rng.uniform(-3.5, 3.5, (n, 100))).astype(np.float32)
        return g(), g()
    if name == "tiny":
        return (rng.standard_normal((n, 100)) * 3e-23).astype(np.float32), np.zeros((n, 100), np.float32)
    scale = dict(edge_of_normal=1e-20, overflow=3e18, near_overflow=1.3e18).get(name)
    if scale is not None:
        return (rng.standard_normal((n, 100)) * scale).astype(np.float32), (rng.standard_normal((n, 100)) * scale).astype(np.float32)
    if name == "non_finite":
        d, q = rng.uniform(-6, 6, (n, 100)).astype(np.float32), rng.uniform(-6, 6, (n, 100)).astype(np.float32)
        plant = np.array([0x7F800000, 0xFF800000, 0x7FC01234, 0x7F7E967A, 0xFF7E967A, 0x80000000], np.uint32).view(np.float32)   # +-3e38
        for i in range(n):
            for _ in range(1 + i % 3):
                (d if rng.random() < 0.5 else q)[i, rng.integers(100)] = plant[rng.integers(plant.size)]
        return d, q
    a, b = T.fp_kat_vectors()                   # the reference's known-answer pair, and its halves swapped
    return np.stack([a[2:], b[2:]]), np.stack([b[2:], a[2:]])


class Dist(Section):
    def __init__(self):
        super().__init__("dist")
        fams = [dist_family(f) for f in DIST_FAMILIES]
        self.D = np.concatenate([f[0] for f in fams])
        self.Q = np.concatenate([f[1] for f in fams])
        self.inputs = {"DIST_D": self.D, "DIST_Q": self.Q}
        lab = ["%s pair %d" % (f, i) for f, fm in zip(DIST_FAMILIES, fams) for i in range(fm[0].shape[0])]
        for nm in ("DIST_PLAIN", "DIST_PK", "DIST_LDS", "DIST_SCALAR"):
            self.labels[nm], self.stride[nm] = lab, 1

    def expected(self, rules=frozenset()):
        simd = dist_keys(dist_simd_order(self.D, self.Q, rules), rules)
        scal = dist_keys(dist_scalar_order(self.D, self.Q, rules - {"dist_tail_into_0_3", "dist_seq_hsum"}), rules)
        m = np.ones(simd.size, bool)
        return {"DIST_PLAIN": (simd, m), "DIST_PK": (simd, m), "DIST_LDS": (simd, m), "DIST_SCALAR": (scal, m)}


# ------------------------------------------------------------------------------------------------------------ predicate
def _f(*bits_or_vals):
    return np.array(bits_or_vals, np.float32)


class Predicate(Section):
    def __init__(self):
        super().__init__("predicate")
        inf, nan = np.inf, np.nan
        q0 = _f(0, 1, 2, 3, 3.999, 4, -0.5, -0.9999, -1, 7.5, 1e9, nan, inf, -inf)
        q1 = _f(5.9, -5.9, 0.0, -0.0, 2147483520, 2147483648, -2147483648, -2147483904, nan, inf, -inf)
        lr = _f([0.3, 0.2], [0.25, 0.25], [nan, 1], [0, nan], [-inf, inf], [inf, -inf], [-0.0, 0.0], [0, 0.5], [nan, nan])
        self.Q = np.array([[a, b, l, r] for a in q0 for b in q1 for l, r in lr], np.float32)
        C = _f(0.0, -0.0, 5, 6, -5, -6, 2147483520, 2147483648, -2147483648, nan, inf, -inf)
        Tt = _f(0.0, -0.0, 0.25, 0.5, 0.2, 0.3, nan, inf, -inf)
        self.rows = np.array([[c, t] for c in C for t in Tt], np.float32)
        fl = np.unique(np.concatenate([self.Q.ravel(), self.rows.ravel()]))
        fl = fl[~np.isnan(fl)]
        fl = np.concatenate([fl[fl < 0], _f(-0.0, 0.0), fl[fl > 0]]).astype(np.float32)       # ascending, -0 in front of +0
        self.ord_f = fl
        self.inputs = {"PRED_Q": self.Q, "PRED_ROWS": self.rows, "ORD_F": fl}
        ql = ["query [%r, %r, %r, %r]" % tuple(float(x) for x in q) for q in self.Q]
        self.labels = {"PRED_PARAMS": ql, "PRED_PASS": ql, "ORD": ["hvs_ordered_u32(%r)" % float(x) for x in fl]}
        self.stride = {"PRED_PARAMS": 4, "PRED_PASS": self.rows.shape[0], "ORD": 1}

    @staticmethod
    def parse(q, rules=frozenset()):
        t, v = float(q[0]), float(q[1])
        if "parse_type_floor" in rules:
            typ = int(np.floor(t)) if -1.0 < t < 4.0 else 4
            typ = typ if 0 <= typ <= 3 else 4
        else:
            typ = int(t) if -1.0 < t < 4.0 else 4                  # truncation toward zero: (-1, 0) is type 0
        if -2147483648.0 <= v < 2147483648.0:
            vf = np.float32(int(np.rint(v)) if "parse_v_rounded" in rules else int(v))
        else:
            vf = np.float32(0)
            typ = 4 if typ in (1, 3) else typ
        return typ, vf, q[2], q[3]

    def expected(self, rules=frozenset()):
        params = np.zeros((self.Q.shape[0], 4), np.uint32)
        passes = np.zeros((self.Q.shape[0], self.rows.shape[0]), np.uint32)
        C, Tt = self.rows[:, 0], self.rows[:, 1]
        with np.errstate(invalid="ignore"):
            for i, q in enumerate(self.Q):
                typ, vf, l, r = self.parse(q, rules)
                params[i] = [typ, f32_bits(vf), f32_bits(l), f32_bits(r)]
                ceq, tin = C == vf, (Tt >= l) & (Tt <= r)
                passes[i] = np.ones_like(ceq) if typ == 0 else ceq if typ == 1 else tin if typ == 2 else ceq & tin if typ == 3 else 0
        u = self.ord_f.view(np.uint32)
        ordv = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
        one = lambda a: (a.ravel(), np.ones(a.size, bool))
        return {"PRED_PARAMS": one(params), "PRED_PASS": one(passes), "ORD": one(ordv)}


# -------------------------------------------------------------------------------------------------------------- the set
class Joined(Section):
    """the instantiations of one section (both NK, both CAP) as one"""

    def __init__(self, name, parts):
        super().__init__(name)
        self.parts = parts
        for p in parts:
            self.inputs.update(p.inputs)
            self.labels.update(p.labels)
            self.stride.update(p.stride)

    def expected(self, rules=frozenset()):
        out = {}
        for p in self.parts:
            out.update(p.expected(rules))
        return out


_sections = None


def sections():
    """{name: Section}, built once"""
    global _sections
    if _sections is None:
        _sections = collections.OrderedDict((s.name, s) for s in (Joined("select", [Select(4), Select(8)]), Joined("cut", [Cut(256), Cut(512)]), PadRank(), Keep(), Gather(), Dedup(), Dist(), Predicate()))
    return _sections


def write_cases(path):
    inputs = {}
    for s in sections().values():
        inputs.update(s.inputs)
    assert set(inputs) == set(IN_BLOBS), set(IN_BLOBS) ^ set(inputs)
    write_blobs(path, [inputs[n] for n in IN_BLOBS])


def compare(section, got, rules=frozenset()):
    """First difference between the harness's output blobs and the model's, as text naming the section, the case and the slot;
    None when every word the contract defines agrees."""
    for name, (want, mask) in section.expected(rules).items():
        have = got[name]
        if have.size != want.size:
            return "%s: %s holds %d words, the model %d" % (section.name, name, have.size, want.size)
        bad = np.nonzero((have != want.astype(have.dtype)) & mask)[0]
        if bad.size:
            w = int(bad[0])
            if name in ("RANK_IDS", "RANK_DISTS"):
                case = int(section.slot_case[w])
                slot = w
            else:
                case, slot = divmod(w, section.stride[name])
            label = section.labels[name][case] if case >= 0 else "(between cases)"
            return "%s: %s case %d [%s] slot %d: got %#x, model %#x (%d words differ)" % (section.name, name, case, label, slot,
                                                                                        int(have[w]), int(want[w]), bad.size)
    return None


# ---------------------------------------------------------------------------------------------------------- the harness
def harness_flags():
    """the engine's own compile flags for a stand-alone program"""
    import importlib
    flags = [f for f in importlib.import_module("project---hybrid-vector-search-queries_amd").engine.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    assert "-ffp-contract=off" in flags, "without it the distance section proves nothing"
    return flags


def build_harness(exe):
    """tests/device_primitives.hip -> exe; returns the compile's wall time in seconds"""
    import os
    import subprocess
    import time
    t0 = time.time()
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + harness_flags() +
                       [os.path.join(T.REPO, "tests", "device_primitives.hip"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return time.time() - t0
