"""Cases and host models for tests/device_index.hip: the index build kernels and the batch layout kernels of csrc/hvs_filter.h,
each launched on its own (tests/test_index_build.py on the GPU, tests/test_index_build_cpu.py for the case set, the wrong
rules and the host functions).

Seeded numpy.  The models follow the kernels' documented contracts (the layout comments of
csrc/hvs_filter.h), not their text; the arithmetic tests/bound_model.py already has is reused (round_up_f32, bf16_round,
f16_round, the rotation matrix, and _int8_model for the closing cross-check).  Where a device sum has a fixed order -- the
100-term row sums of the plain builders and of hvs_k_plan_stats, the 100-term sums of hvs_rot_elem -- the model adds in that
order in f64 (seq_sum, rotate_seq), so those values are compared bit for bit.

Sections, in the harness's order: keys, quant, tiles, patch, plan, batch, prep.  The blob format, its reader and its writer are those
of tests/primitives_model.py.

What is compared, and how (check_* below):
* word for word: keys, ids, blockpos, every tile byte, the accumulator inits of the plain INT8 builders, the padding and the
  tombstone encodings, `patched`, kmin, kmax, center, sd, inv_sd, rot, hmax, rho, pair_n, class counts, query keys, ranges and
  the whole slot layout (the same words from one, two and three workgroups).
* behind a device sqrt (e_d, nb_d, e_d8, n_d8, e_df, nb_df; eq, nqb and the 16-bit formats' normq of hvs_k_prep): at or above the exact f64 value, and at most one f32 ulp above the
  model's rounded-up value; check_* counts the values that differ from the model at all.
* order-dependent f64 sums (the LDS atomicAdd sums of hvs_k_build_tiles_i8x16_rot and of rotated hvs_k_prep, pair_sum, pair_sumsq): within 1e-12
  relative; an accumulator init derived from one must be floor(v) for a v within that distance of the model's un-floored value.

Every model takes a set of WRONG RULES (RULES below), one plausible mistake each; test_index_build_cpu.py shows that each
changes an expected word of some case.
"""
import os
import subprocess
import time

import numpy as np

import bound_model as BM
import hvs_testlib as T
import primitives_model as P

NDIM, RDIM, DCOLS, QCOLS = 100, 128, 102, 104
PAD_NORM = -(1 << 30)
GROUP, WG_WAVES = 128, 4
QUANT_WORDS, BOUNDS_WORDS, LEVELS_WORDS = 390, 14, 83
CASE_N = (1, 31, 33, 33, 4100)
CASE_NAMES = ("one_row", "equal_rows", "f16_edges", "non_finite", "levels")
FLAG_TILES, FLAG_F16 = 1, 2
CASE_FLAGS = (FLAG_TILES | FLAG_F16, FLAG_TILES | FLAG_F16, FLAG_TILES, 0, FLAG_TILES | FLAG_F16)
BATCH_CASE = 4
BUILDERS = ("bf16", "f16", "i8", "i8x16", "rot")
PATCH_FORMATS = ("bf16", "f16", "i8", "i8x16")
TILE_WORDS = dict(bf16=7 * 64 * 4, f16=7 * 64 * 4, i8=3 * 64 * 4, i8x16=4 * 64 * 4, rot=4 * 64 * 4)     # per block
NORM_WORDS = dict(bf16=0, f16=0, i8=64, i8x16=32, rot=32)
SQRT_BOUNDS = (0, 1, 4, 5, 6, 7)      # e_d, nb_d, e_d8, n_d8, e_df, nb_df of HvsBounds
BOUND_NAMES = ("e_d", "nb_d", "hmax", "rho", "e_d8", "n_d8", "e_df", "nb_df")

RULES = {
    "keys": ("key_nan_not_largest", "key_neg_zero_unfolded"),
    "quant": ("center_f64", "scale_no_slack", "rot_box_inward"),
    "tiles": ("nh_ceil", "nh_round", "pad_no_bias", "invalid_takes_perm0", "kpad_nonzero", "i8x16_lane_shift5", "frag_swapped",
              "h1_from_hf", "h_pieces_shifted"),
    "patch": ("tombstone_h0_wrong_word",),
    "batch": ("type3_upper_no_plus1", "type1_ends_at_nan", "class_pad_64", "t_part_group_aligned", "layout6_in_slots"),
    "prep": ("quant_half_away", "quant_clamp_128", "bfrag_ones_k_lt_102", "hopeless_2x", "eq_counts_clipped", "clip_wrong_half",
             "f16_flush_left_out", "cap_nothing_keeps_all", "capped_theta_from_inf", "theta_from_wrong_norm", "bfrag_lane_shift5",
             "bfrag_index_swapped"),
}
# Round-half-away and a clamp at +-128 are switches of the QUERY side only (prep): on rows sd = max |d'_k| / 127 (1 + 1e-9) keeps
# every |d'_k| / sd below 127.5, and a row component whose f64 quotient is exactly j + 1/2 needs an f32 input inside a 2^-52 window.
_u32, _u64, _f32, _f64 = np.uint32, np.uint64, np.float32, np.float64


# ------------------------------------------------------------------------------------------------------- host functions
def attr_key(f, rules=frozenset()):
    """hvs_attr_key: "-0 is folded into +0 ..., NaN maps to the largest key" """
    f = np.ascontiguousarray(f, _f32)
    u = f.view(_u32)
    if "key_neg_zero_unfolded" not in rules:
        u = np.where(f == 0, _u32(0), u)
    k = np.where((u & _u32(0x80000000)) != 0, ~u, u | _u32(0x80000000)).astype(_u32)
    if "key_nan_not_largest" not in rules:
        k = np.where(np.isnan(f), _u32(0xFFFFFFFF), k)
    return k.astype(_u32)


def attr_key_inv(k):
    k = np.asarray(k, _u32)
    return np.where((k & _u32(0x80000000)) != 0, k & _u32(0x7FFFFFFF), ~k).astype(_u32).view(_f32)


def host_floats():
    t = [0, 0x80000000, 1, 0x80000001, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00800000, 0x80800000]
    return np.array(t + [(i * 2654435761) & 0xFFFFFFFF for i in range(4096)], _u32)


class Levels:
    """hvs_make_levels: "Radices (powers of two) from the last level backwards: r_last, then r_mid, ..., each cut down so that
    level 0 keeps >= 16 blocks"; level j holds "the multiples of stride[j] not in an earlier level" """

    def __init__(self, n, r_last=4, r_mid=16):
        self.n, self.nblk = n, (n + 31) // 32
        rad, S = [], 1
        while True:
            r = r_last if not rad else r_mid
            while r >= 2 and self.nblk // (S * r) < 16:
                r >>= 1
            if r < 2 or len(rad) >= 14:
                break
            rad.append(r)
            S *= r
        K = self.K = len(rad)
        self.stride, self.radix, self.off = [1] * 16, [2] * 16, [0] * 16
        self.radix[0] = 1
        for j in range(K, 0, -1):
            self.radix[j] = rad[K - j]
            self.stride[j - 1] = self.stride[j] * self.radix[j]
        self.blocks, off = [], 0                     # blocks in storage order, from the definition of the levels
        for j in range(K + 1):
            self.off[j] = off
            mine = [b for b in range(0, self.nblk, self.stride[j]) if j == 0 or b % self.stride[j - 1] != 0]
            self.blocks += mine
            off += len(mine)
        for j in range(K + 1, 16):
            self.off[j] = off
        self.level_of = np.repeat(np.arange(K + 1), np.diff(self.off[:K + 2]))
        self.blocks = np.array(self.blocks, np.int64)

    def words(self):
        lg = lambda v: [int(x).bit_length() - 1 for x in v]
        return np.array([self.K, self.nblk] + self.off + self.stride + self.radix + lg(self.stride) + lg(self.radix) + [1], _u32)


_levels = {}


def levels(n):
    if n not in _levels:
        _levels[n] = Levels(n)
    return _levels[n]


# ------------------------------------------------------------------------------------------------------------ arithmetic
def seq_sum(a):
    """the rows' sums in the device's order: s = s + a[:, k] for k = 0, 1, ..."""
    s = np.zeros(a.shape[0], _f64)
    for k in range(a.shape[1]):
        s = s + a[:, k]
    return s


_R = None


def rotate_seq(x):
    """hvs_rot_elem: a += +-x_j for j = 0 .. 99 in order, then a / sqrt(128): [n, 100] f32 -> [n, 128] f64"""
    global _R
    if _R is None:
        _R = BM.rot_matrix()
    x = np.asarray(x, _f32).astype(_f64)
    a = np.zeros((x.shape[0], RDIM), _f64)
    with np.errstate(invalid="ignore"):
        for j in range(NDIM):
            a = a + x[:, j:j + 1] * _R[None, :, j]
    return a * 0.08838834764831844055


def h16_bits(fmt, x):
    x = np.ascontiguousarray(x, _f32)
    if fmt == "f16":
        with np.errstate(over="ignore"):
            return x.astype(np.float16).view(np.uint16)
    return (BM.bf16_round(x).view(_u32) >> 16).astype(np.uint16)


def h16_val(fmt, b):
    b = np.asarray(b, np.uint16)
    return b.view(np.float16).astype(_f32) if fmt == "f16" else (b.astype(_u32) << 16).view(_f32)


class Quant:
    """HvsQuant after hvs_k_quant_reset, hvs_k_minmax(_rot) and hvs_k_quant_params"""

    def __init__(self, V, rot, rules=frozenset()):
        self.rot, self.nd = int(rot), RDIM if rot else NDIM
        kmin, kmax = np.full(RDIM, 0xFFFFFFFF, _u32), np.zeros(RDIM, _u32)
        with np.errstate(all="ignore"):
            if rot:   # "f32 neighbours of a double, rounded outward (the box of the rotated data must contain every rotated row)"
                self.X = rotate_seq(V)
                lo_f, hi_f = BM._f32_below(self.X), BM._f32_above(self.X)
                if "rot_box_inward" in rules:
                    lo_f, hi_f = hi_f, lo_f
                kmin, kmax = attr_key(lo_f).min(0), attr_key(hi_f).max(0)
            else:
                self.X = np.asarray(V, _f32).astype(_f64)
                k = attr_key(V)
                kmin[:NDIM], kmax[:NDIM] = k.min(0), k.max(0)
            lo, hi = attr_key_inv(kmin[:self.nd]).astype(_f64), attr_key_inv(kmax[:self.nd]).astype(_f64)
            mid = 0.5 * (lo + hi)
            c = mid.astype(_f32)                                    # "centre c (midrange of D)", an f32
            c_used = mid if "center_f64" in rules else c.astype(_f64)
            a, b = np.abs(lo - c_used), np.abs(hi - c_used)
            half = np.where(np.isnan(a) | np.isnan(b), np.inf, np.maximum(a, b))
        m = float(half.max()) if half.max() > 0 else 0.0
        sd = 1.0 if not m > 0.0 else (m / 127.0 if "scale_no_slack" in rules else m / 127.0 * (1.0 + 1e-9))
        if not sd < 1.0e18 or sd < 1.0e-18:
            sd = 0.0                                                # "non-finite or extreme ranges: INT8 format unusable"
        self.kmin, self.kmax, self.half = kmin, kmax, half
        self.center = np.zeros(RDIM, _f32)
        self.center[:self.nd] = c
        self.sd, self.inv_sd = sd, (1.0 / sd if sd > 0.0 else 0.0)

    def words(self):
        w = np.zeros(QUANT_WORDS, _u32)
        w[0:128] = self.center.view(_u32)
        w[128:132] = np.array([self.sd, self.inv_sd], _f64).view(_u32)
        w[132:260], w[260:388], w[388] = self.kmin, self.kmax, self.rot
        return w


def quant_i8(x, inv_sd, rules=frozenset()):
    """dq = clamp(rint(d'/sd), +-127), a NaN as 0"""
    lim = 128.0 if "quant_clamp_128" in rules else 127.0
    with np.errstate(invalid="ignore"):
        t = x * inv_sd
        r = np.sign(t) * np.floor(np.abs(t) + 0.5) if "quant_half_away" in rules else np.rint(t)
        r = np.clip(r, -lim, lim)
    return np.where(np.isnan(r), 0.0, r)


def i8_rows(qz, rules=frozenset()):
    """-> dq [n, 128] (zeros behind the space's dimensions), nd, e2 (the row sums in k order), v (the un-floored init)"""
    x = qz.X - qz.center[:qz.nd].astype(_f64)
    dq = quant_i8(x, qz.inv_sd)
    d = x - qz.sd * dq
    nd, e2 = seq_sum(x * x), seq_sum(d * d)
    v = -0.5 * nd * qz.inv_sd * qz.inv_sd
    out = np.zeros((x.shape[0], RDIM), _f64)
    out[:, :qz.nd] = dq
    if "kpad_nonzero" in rules and qz.nd < RDIM:
        out[:, qz.nd:] = 1.0
    return out, nd, e2, v


def nh_of(v, rules=frozenset()):
    """nh = floor(-|d'|^2 / (2 sd^2)); beyond -1e9 the padding value"""
    f = np.ceil(v) if "nh_ceil" in rules else np.rint(v) if "nh_round" in rules else np.floor(v)
    return np.where(f > -1.0e9, f, PAD_NORM).astype(np.int64)


def bound_exact(s2, flush=0.0, slack=True):
    """the f64 value a row bound rounds up from"""
    with np.errstate(invalid="ignore"):
        r = np.sqrt(s2)
    return r * (1.0 + 1e-9) + 1e-30 if slack else r + flush


def h16_rows(fmt, V, rules=frozenset()):
    """-> image [n, 112] u16 of the valid rows (components, then -|d|^2/2 "split into three pieces" at k = 100..102), and the
    rows' bound terms"""
    V = np.asarray(V, _f32)
    x = V.astype(_f64)
    bits = h16_bits(fmt, V)
    xb = h16_val(fmt, bits).astype(_f64)
    with np.errstate(all="ignore"):
        nd, e2, nb2 = seq_sum(x * x), seq_sum((x - xb) * (x - xb)), seq_sum(xb * xb)
        hf = (-0.5 * nd).astype(_f32)
        h0 = h16_bits(fmt, hf)
        r1 = (hf - h16_val(fmt, h0)).astype(_f32)
        h1 = h16_bits(fmt, hf if "h1_from_hf" in rules else r1)
        r2 = (r1 - h16_val(fmt, h1)).astype(_f32)
        h2 = h16_bits(fmt, r2)
        hs = h16_val(fmt, h0).astype(_f64) + h16_val(fmt, h1).astype(_f64) + h16_val(fmt, h2).astype(_f64)
        rho = np.abs(0.5 * nd + hs) + (BM.F16_FLUSH_RHO if fmt == "f16" else 0.0) + 1e-30
    img = np.zeros((V.shape[0], 112), np.uint16)
    img[:, :NDIM] = bits
    ks = (101, 100, 102) if "h_pieces_shifted" in rules else (100, 101, 102)
    img[:, ks[0]], img[:, ks[1]], img[:, ks[2]] = h0, h1, h2
    return img, dict(nd=nd, e2=e2, nb2=nb2, rho=rho)


def h16_pad_image(fmt, rules=frozenset(), k0=100):
    """a padding row, and a tombstone: "components zero, h0 = the padding bias, h1 = h2 = 0" """
    img = np.zeros(112, np.uint16)
    if "pad_no_bias" not in rules:
        img[k0] = h16_bits(fmt, np.array([-65504.0 if fmt == "f16" else -1.0e30], _f32))[0]
    return img


# ---------------------------------------------------------------------------------------------------------- tile layouts
# (lane, byte) -> (row of the block, k), written from the layout comments of csrc/hvs_filter.h
def _map_h16():      # "element k = 16 s + 8 h + 2 p + e of the row", lane = (row l & 31, half h = l >> 5); 8 elements per lane
    s, l, j = np.meshgrid(np.arange(7), np.arange(64), np.arange(8), indexing="ij")
    return l & 31, 16 * s + 8 * (l >> 5) + j


def _map_i8():       # "lane l of k-step s: row l&31, k = 32 s + 16 (l>>5) + 0..15; k-steps 0..2"
    s, l, j = np.meshgrid(np.arange(3), np.arange(64), np.arange(16), indexing="ij")
    return l & 31, 32 * s + 16 * (l >> 5) + j


def _map_i8x16(rules=frozenset()):   # "fragment f = 2 rb + ks; lane l: row 16 rb + (l & 15), k = 64 ks + 16 (l >> 4) + 0..15"
    f, l, j = np.meshgrid(np.arange(4), np.arange(64), np.arange(16), indexing="ij")
    rb, ks = (f & 1, f >> 1) if "frag_swapped" in rules else (f >> 1, f & 1)
    sh = 5 if "i8x16_lane_shift5" in rules else 4
    return 16 * rb + (l & 15), 64 * ks + 16 * (l >> sh) + j


def tile_map(b, rules=frozenset()):
    return _map_h16() if b in ("bf16", "f16") else _map_i8() if b == "i8" else _map_i8x16(rules)


def describe_tile_word(b, word):
    """storage index, fragment, lane, word and the (row, k) range a tile word holds"""
    idx, w = divmod(int(word), TILE_WORDS[b])
    s, r = divmod(w, 256)
    lane, p = divmod(r, 4)
    row, k = tile_map(b)
    per = 8 if b in ("bf16", "f16") else 16
    j0 = p * (2 if per == 8 else 4)
    return "storage index %d fragment %d lane %d word %d = row %d of the block, k %d..%d" % (
        idx, s, lane, p, row[s, lane, j0], k[s, lane, j0], k[s, lane, j0] + (1 if per == 8 else 3))


class Built:
    """what one builder leaves for both orderings: tiles, norms, blockpos per ordering, the raised bounds, and for the
    order-dependent rot builder the un-floored inits"""


def build_model(case, b, rules=frozenset(), dead=None):
    """`dead` (bool per row id): the tiles after hvs_k_patch_tiles under that mask"""
    L, n = levels(case.n), case.n
    fmt = b
    out = Built()
    out.tiles, out.norms, out.bpos, out.vfloat = [], [], [], []
    bounds = np.zeros(8, _f32)
    exact = np.zeros(8, _f64)
    if b in ("bf16", "f16"):
        img_rows, tr = h16_rows(fmt, case.V, rules)
        pad = h16_pad_image(fmt, rules)
        tomb = h16_pad_image(fmt, frozenset(), 98 if "tombstone_h0_wrong_word" in rules else 100)
        with np.errstate(all="ignore"):
            ex = dict(e_d=bound_exact(tr["e2"], BM.F16_FLUSH if fmt == "f16" else 0.0, False), nb_d=bound_exact(tr["nb2"], 0.0, False),
                      hmax=0.5 * tr["nd"], rho=tr["rho"])
        for i, nm in enumerate(("e_d", "nb_d", "hmax", "rho")):
            exact[i], bounds[i] = ex[nm].max(), BM.round_up_f32(ex[nm]).max()
    else:
        qz = case.quant(b == "rot", rules)
        dq, nd, e2, v = i8_rows(qz, rules)
        nh_rows = nh_of(v, rules)
        img_rows = dq.astype(np.int8).view(np.uint8)
        ex = dict(e_d8=bound_exact(e2), n_d8=bound_exact(nd))
        for i, nm in ((4, "e_d8"), (5, "n_d8")):
            exact[i], bounds[i] = ex[nm].max(), BM.round_up_f32(ex[nm]).max()
    row, k = tile_map(b, rules)
    pos = L.blocks[:, None] * 32 + np.arange(32)[None, :]            # [storage index, row of the block]
    valid = pos < n
    for o in range(2):
        rid = case.perm[o][np.where(valid, pos, 0)]
        img = img_rows[rid].copy()                                   # [idx, 32, K]
        if b in ("bf16", "f16"):
            if "invalid_takes_perm0" in rules:
                img[~valid, 100:103] = pad[100:103]
            else:
                img[~valid] = pad
            if dead is not None:
                img[valid & dead[rid]] = tomb
            t = img[:, row, k]                                       # [idx, 7, 64, 8] u16
            out.norms.append(np.zeros(0, _u32))
        else:
            if "invalid_takes_perm0" not in rules:
                img[~valid] = 0
            nh = np.where(valid, nh_rows[rid], 0 if "pad_no_bias" in rules else PAD_NORM)
            vf = np.where(valid, v[rid], np.nan)
            if dead is not None:
                nh = np.where(valid & dead[rid], PAD_NORM, nh)
                vf = np.where(valid & dead[rid], np.nan, vf)
            nh32 = nh.astype(np.int32).view(_u32)
            t = img[:, row, k]
            if b == "i8":   # side data: "[0,8) dims 96..99 of the 32 rows (4 x int8 each), [8,16) the rows' accumulator inits"
                tail = np.ascontiguousarray(img[:, :, 96:100]).view(_u32)[:, :, 0]
                out.norms.append(np.concatenate([tail, nh32], 1).ravel())
            else:
                out.norms.append(nh32.ravel())
            out.vfloat.append(vf.ravel())
        out.tiles.append(np.ascontiguousarray(t).view(_u32).ravel())
        out.bpos.append(L.blocks.astype(_u32))
    out.bounds, out.exact = bounds, exact
    return out


def plan_model(case, step):
    """HvsBounds after hvs_k_plan_stats: the bounds both formats would get from the sampled rows, and the pair statistics"""
    n, V = case.n, case.V
    i = np.arange(0, n, step, dtype=np.int64)
    j = (i * 2654435761 + 40503) % n
    qz = case.quant(False)
    x = V[i].astype(_f64)
    out = dict(f=np.zeros(8, _f32), exact=np.zeros(8, _f64), pair_n=0, pair_sum=0.0, pair_sumsq=0.0)
    with np.errstate(all="ignore"):
        xb, xf = h16_val("bf16", h16_bits("bf16", V[i])).astype(_f64), h16_val("f16", h16_bits("f16", V[i])).astype(_f64)
        nd, e2, nb2 = seq_sum(x * x), seq_sum((x - xb) * (x - xb)), seq_sum(xb * xb)
        e2f, nb2f = seq_sum((x - xf) * (x - xf)), seq_sum(xf * xf)
        x8 = x - qz.center[:NDIM].astype(_f64)
        d8 = x8 - qz.sd * quant_i8(x8, qz.inv_sd)
        nd8, e28 = seq_sum(x8 * x8), seq_sum(d8 * d8)
        df = x - V[j].astype(_f64)
        dist = seq_sum(df * df)
        ok = nd < 1.0e30
        okf = ok & (nb2f < 1.0e30)
        terms = {0: (np.sqrt(e2), ok), 1: (np.sqrt(nb2), ok), 2: (0.5 * nd, ok), 4: (np.sqrt(e28), ok), 5: (np.sqrt(nd8), ok),
                 6: (np.sqrt(e2f) + BM.F16_FLUSH, okf), 7: (np.sqrt(nb2f), okf)}
        for s, (val, m) in terms.items():
            if m.any():
                out["exact"][s], out["f"][s] = val[m].max(), BM.round_up_f32(val[m]).max()
        if (ok & ~okf).any():
            out["f"][7] = out["exact"][7] = np.inf      # "a component beyond the half-precision range: F16 unusable"
        pm = ok & (i != j) & (dist < 1.0e30)
        out["pair_n"], out["pair_sum"], out["pair_sumsq"] = int(pm.sum()), float(dist[pm].sum()), float((dist[pm] * dist[pm]).sum())
    return out


# ------------------------------------------------------------------------------------------------------------------ cases
class Case:
    def __init__(self, name, D, dead_ids):
        self.name, self.D, self.n = name, np.ascontiguousarray(D, _f32), D.shape[0]
        self.V = self.D[:, 2:]
        self.dead = np.zeros(self.n, bool)
        self.dead[np.asarray(dead_ids, np.int64)] = True
        self._q, self._keys = {}, {}

    def keys(self, rules=frozenset()):
        """keys_ct, keys_t, ids, and the two orderings: by (C, T) with ties by id, by (T, id)"""
        key = frozenset(rules) & set(RULES["keys"])
        if key not in self._keys:
            kc, kt = attr_key(self.D[:, 0], rules).astype(_u64), attr_key(self.D[:, 1], rules).astype(_u64)
            ids = np.arange(self.n, dtype=_u64)
            kct, ktt = (kc << _u64(32)) | kt, (kt << _u64(32)) | ids
            self._keys[key] = (kct, ktt, ids.astype(_u32), np.lexsort((ids, kct)), np.argsort(ktt, kind="stable"))
        return self._keys[key]

    @property
    def perm(self):
        return self.keys()[3:5]

    def quant(self, rot, rules=frozenset()):
        key = (bool(rot), frozenset(rules) & set(RULES["quant"]))
        if key not in self._q:
            self._q[key] = Quant(self.V, rot, key[1])
        return self._q[key]

    def live_words(self):
        bits = np.zeros(((self.n + 31) // 32) * 32, np.uint8)
        bits[:self.n] = ~self.dead
        return np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view(_u32).ravel()

    def inputs(self, flags):
        return [self.D, np.concatenate(self.perm).astype(_u32), self.live_words(), np.array([flags], _u32)]


def _attrs(rng, n):
    """C and T with the edges: C = -0.0 beside +0.0, T = NaN rows, duplicate (C, T) pairs"""
    C = rng.integers(0, 6, n).astype(_f32)
    Tt = np.round(rng.uniform(0, 1000, n), 0).astype(_f32)          # whole numbers: many equal T, some equal (C, T)
    C[rng.random(n) < 0.1] = -0.0
    Tt[rng.random(n) < 0.05] = np.nan
    Tt[rng.random(n) < 0.03] = -0.0
    return C, Tt


def _make_cases():
    rng = np.random.default_rng(2024)
    cases = []
    # one row: every dimension constant, scale 1
    D = np.zeros((1, DCOLS), _f32)
    D[0, :2], D[0, 2:] = (3.0, np.nan), rng.normal(0, 2, NDIM)
    cases.append(Case(CASE_NAMES[0], D, [0]))
    # 31 equal rows (scale 1), one partial block; the dead rows leave live ones beside them
    D = np.zeros((31, DCOLS), _f32)
    D[:, 0], D[:, 1] = _attrs(rng, 31)
    D[:, 2:] = (np.round(rng.normal(0, 3, NDIM) * 8) / 8).astype(_f32)[None, :]      # on a grid of 1/8: see PrepSet 1
    cases.append(Case(CASE_NAMES[1], D, [0, 7, 30]))
    # 33 rows, two blocks, K = 0: half-precision edges (the denormal boundary 2^-14 and its neighbours, denormals, a component
    # beyond 65504 -- the planner then rules F16 out, so the F16 builder is not run on this case), -0.0, a constant dimension
    D = np.zeros((33, DCOLS), _f32)
    D[:, 0], D[:, 1] = _attrs(rng, 33)
    D[:, 2:] = rng.normal(0, 1, (33, NDIM))
    b = _f32(2.0 ** -14)
    D[3, 2:8] = [b, np.nextafter(b, _f32(0)), np.nextafter(b, _f32(1)), -b, _f32(2.0 ** -15), _f32(2.0 ** -25)]
    D[5, 10], D[6, 11], D[:, 20], D[8, 30] = 70000.0, -0.0, 0.75, 65504.0
    cases.append(Case(CASE_NAMES[2], D, [32]))
    # non-finite components: only hvs_k_attr_keys and set_quant's kernels are modelled on it (sd = 0: no INT8 format)
    D = np.zeros((33, DCOLS), _f32)
    D[:, 0], D[:, 1] = _attrs(rng, 33)
    D[:, 2:] = rng.normal(0, 1, (33, NDIM))
    D[4, 2], D[9, 3], D[11, 4], D[1, 0], D[2, 0] = np.nan, np.inf, -np.inf, np.nan, np.inf
    cases.append(Case(CASE_NAMES[3], D, []))
    # 4100 rows: three levels, radices 2 and 4, a partial last block that is not the last storage index.  A PCA-like spectrum
    # (so that the rotated box differs from the plain one), then edge rows: both box extremes in every dimension, rows half a
    # quantisation step off the grid (the nearest f32 and its neighbours), a constant dimension.
    n = CASE_N[4]
    D = np.zeros((n, DCOLS), _f32)
    D[:, 0], D[:, 1] = _attrs(rng, n)
    spec = 4.0 * 0.93 ** np.arange(NDIM)
    V = rng.normal(0, 1, (n, NDIM)) * spec[None, :] + rng.normal(0, 1, NDIM)[None, :]
    V[:, 57] = 1.25
    D[:, 2:] = V
    tmp = Case("tmp", D, [])
    lo, hi = tmp.V.min(0).astype(_f64), tmp.V.max(0).astype(_f64)
    D[10, 2:], D[11, 2:] = lo, hi                                  # (they are the extremes already: the box stays)
    qz = Case("tmp", D, []).quant(False)
    c = qz.center[:NDIM].astype(_f64)
    for r, jj in ((20, 3), (21, -7), (22, 40), (23, -126)):
        t = (c + (jj + 0.5) * qz.sd).astype(_f32)
        t = np.clip(t, lo.astype(_f32), hi.astype(_f32))
        D[r, 2:] = t
        D[r + 10, 2:] = np.clip(np.nextafter(t, _f32(np.inf)), lo.astype(_f32), hi.astype(_f32))
        D[r + 20, 2:] = np.clip(np.nextafter(t, _f32(-np.inf)), lo.astype(_f32), hi.astype(_f32))
    D[60:64, 0], D[60:64, 1] = 2.0, 5.0                            # duplicate (C, T) pairs: their order is by id
    L = levels(n)
    ct = np.lexsort((np.arange(n), (attr_key(D[:, 0]).astype(_u64) << _u64(32)) | attr_key(D[:, 1]).astype(_u64)))
    # dead rows: in the first block and in the partial last block, a whole block (block 5 of the (C, T) ordering), none in others
    dead = [int(ct[0]), int(ct[17]), int(ct[n - 1]), int(ct[n - 3])] + [int(x) for x in ct[5 * 32:6 * 32]]
    cases.append(Case(CASE_NAMES[4], D, dead))
    assert tuple(c.n for c in cases) == CASE_N and L.K >= 2
    return cases


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = _make_cases()
    return _cases


# ------------------------------------------------------------------------------------------------------------------ batch
def type_rank(t):
    return {0: 0, 1: 1, 3: 2, 2: 4}.get(t, 3)


def query_range(p, kct, ktt, n, rules=frozenset()):
    """hvs_query_range: "type 0 = everything, type 1 = the C==v run, type 3 = the T-window inside that run, type 2 = a T-window
    of the T ordering"; "NaN bounds match nothing"; "rows with T = NaN still match C==v".  Two searchsorted calls on the keys."""
    typ, vf, l, r = p
    kv, kl, kr = (int(attr_key(np.array([x], _f32))[0]) for x in (vf, l, r))
    ok = not (np.isnan(l) or np.isnan(r)) and kl <= kr
    plus = 0 if "type3_upper_no_plus1" in rules else 1
    a = b = 0
    if typ == 0:
        b = n
    elif typ == 1:
        a = np.searchsorted(kct, _u64(kv << 32), "left")
        b = np.searchsorted(kct, _u64((kv << 32) | 0xFFFFFFFE), "right") if "type1_ends_at_nan" in rules else \
            (np.searchsorted(kct, _u64((kv + 1) << 32), "left") if kv < 0xFFFFFFFF else n)
    elif typ == 3 and ok:
        a = np.searchsorted(kct, _u64((kv << 32) | kl), "left")
        b = np.searchsorted(kct, _u64((kv << 32) + kr + plus), "left")
    elif typ == 2 and ok:
        a = np.searchsorted(ktt, _u64(kl << 32), "left")
        b = np.searchsorted(ktt, _u64((kr + plus) << 32), "left") if kr + plus <= 0xFFFFFFFF else n
    a, b = int(a), int(b)
    return a, max(a, b)


def nbins_of(count):
    """"as many start-position bins as there are quads of 512 queries per bin": floor(sqrt(count / 512)) in f32, in [1, 4096]"""
    v = int(np.sqrt(_f32(count) * _f32(1.0 / 512.0), dtype=_f32))
    return min(max(v, 1), 4096)


# The class populations behind the synthetic bins: 1 bin, 2, a mid value, and the most a 32-bit population can give.  (The
# kernel's clamp at 4096 bins would need 2^33 queries of one class: no batch reaches it, so no case does.)
SYN_COUNTS = np.array([[100, 2048 + 5, 9 * 512 + 100, 3, 700], [0xFFFFFFFF] * 5, [2048 + 5] * 5], _u32)


class Batch:
    """count_classes, query_keys2 and layout on the big case, in the q0 + range form and in the list form"""

    def __init__(self):
        rng = np.random.default_rng(77)
        case = cases()[BATCH_CASE]
        n = case.n
        kct, ktt = case.keys()[0], case.keys()[1]
        self.kct, self.ktt, self.n = np.sort(kct), np.sort(ktt), n
        D = case.D
        rows = []

        def add(typ, v=-1.0, l=-1.0, r=-1.0):
            rows.append([typ, v, l, r])
        # class populations of the range form (queries q0 .. q0 + nq_range): type 0: 33, type 1: 32, type 3: 31, invalid: 1,
        # type 2: 600 (pushes nothing; the T part must start at the next multiple of 512 slots)
        for _ in range(33):
            add(0)
        for i in range(32):
            add(1, float(i % 7))                      # C = 6 has no row: an empty range
        t3 = [(0.0, 100.0, 400.0), (1.0, 400.0, 100.0), (2.0, np.nan, 5.0), (2.0, 5.0, np.nan), (2.0, 5.0, 5.0), (0.0, -np.inf, np.inf),
              (-0.0, 0.0, 0.0), (3.0, -0.0, 1000.0), (9.0, 0.0, 1000.0)]
        for i in range(31):
            v, l, r = t3[i] if i < len(t3) else (float(rng.integers(0, 6)), *np.sort(rng.uniform(0, 1000, 2)))
            add(3, v, l, r)
        add(7)                                        # an invalid type
        for i in range(600):
            l, r = np.sort(rng.uniform(-50, 1050, 2))
            add(2, -1.0, l, r)
        rows[97 + 0][2:] = [-np.inf, np.inf]          # type 2: the whole ordering but its NaN rows
        rows[97 + 1][2:] = [5.0, 5.0]
        rows[97 + 2][2:] = [700.0, 100.0]
        rows[97 + 3][2:] = [np.nan, np.nan]
        self.nq_range = len(rows)
        # behind them, queries only the list form uses
        for _ in range(40):
            add(1, float(rng.integers(0, 6)))
        add(4.5), add(-3.0), add(np.nan), add(1, 3.0e9)
        self.q0 = 3
        Q = np.zeros((self.q0 + len(rows), QCOLS), _f32)
        Q[:self.q0, 0] = 1.0
        Q[self.q0:, :4] = np.array(rows, _f32)
        # vectors: rows of the data with a little noise (inside the box or a hair outside), then the edges on type-0 queries
        Q[:, 4:] = case.V[rng.integers(0, n, Q.shape[0])] + rng.normal(0, 0.3, (Q.shape[0], NDIM)).astype(_f32)
        qz = case.quant(False)
        c, sd = qz.center[:NDIM].astype(_f64), qz.sd
        e = self.q0
        self.edge = dict(centre=e, just_outside=e + 1, far_outside=e + 2, nan=e + 3, huge=e + 4, past_half=e + 5, between_2x_4x=e + 8, just_outside_t2=e + 120)
        Q[e, 4:] = c
        for qi in (e + 1, e + 120):
            Q[qi, 4:] = Q[e + 7, 4:]
            Q[qi, 4 + 10:4 + 13] = (c[10:13] + 128.2 * sd).astype(_f32)
        Q[e + 2, 4:24] = (c[:20] + 2000.0 * sd).astype(_f32)
        Q[e + 8, 4:] = Q[e + 7, 4:]
        Q[e + 8, 4 + 10:4 + 13] = (c[10:13] + 161.0 * sd).astype(_f32)         # a clip term between 2x and 4x the rest of the band
        Q[e + 3, 4 + 50], Q[e + 4, 4 + 60], Q[e + 5, 4 + 70] = np.nan, 1.0e16, 70000.0
        self.Q = Q
        # the list form: class populations 0 (type 0), 33 (type 1), 1 (type 3), 4 (invalid) and a type-2 part of 32
        nq = Q.shape[0]
        typ = np.array([type_rank(P.Predicate.parse(q)[0]) for q in Q])
        pick = lambda rk, c: rng.permutation(np.nonzero(typ == rk)[0])[:c]
        self.list = rng.permutation(np.concatenate([pick(1, 33), pick(2, 1), pick(3, 4), pick(4, 32)])).astype(_u32)
        assert self.list.max() < nq
        self.forms = [self._form(np.arange(self.q0, self.q0 + self.nq_range)), self._form(self.list.astype(np.int64))]

    def _form(self, qis, rules=frozenset()):
        f = dict(qis=qis, nqb=len(qis))
        par = [P.Predicate.parse(self.Q[qi]) for qi in qis]
        rk = np.array([type_rank(p[0]) for p in par])
        f["rank"] = rk
        f["counts"] = np.bincount(rk, minlength=5).astype(_u32)
        ab = np.array([query_range(p, self.kct, self.ktt, self.n, rules) for p in par], np.int64).reshape(-1, 2)
        f["qa"], f["qb"] = ab[:, 0].astype(_u32), ab[:, 1].astype(_u32)
        f["keys"] = self.keys_for(f, f["counts"])
        f["idx"] = np.arange(len(qis), dtype=_u32)
        order = np.argsort(f["keys"], kind="stable")
        f["sorted_keys"], f["sorted_idx"] = f["keys"][order], order.astype(_u32)
        f["nslots"] = -(-(len(qis) + 5 * 32 + (WG_WAVES + 1) * GROUP) // GROUP) * GROUP
        return f

    def keys_for(self, f, counts):
        """"rank:3 | bin of the range start:12 | range end:32" """
        nb = np.array([nbins_of(int(counts[r])) for r in f["rank"]], np.int64)
        abin = (f["qa"].astype(np.int64) * nb) // (self.n + 1)
        return (f["rank"].astype(_u64) << _u64(61)) | (abin.astype(_u64) << _u64(32)) | f["qb"].astype(_u64)

    def layout(self, f, rules=frozenset()):
        """"each class padded to whole 32-slot blocks, the (C,T) part padded to a whole quad of groups ..., the type-2 part to a
        whole group.  layout[0..4] = first slot of each class rank, layout[5] = nslots used, layout[6] = first group of T part" """
        ns, cnt = f["nslots"], f["counts"].astype(np.int64)
        padto = 64 if "class_pad_64" in rules else 32
        tal = GROUP if "t_part_group_aligned" in rules else WG_WAVES * GROUP
        slot0, s = [], 0
        for rk in range(5):
            if rk == 4:
                s = -(-s // tal) * tal
            slot0.append(s)
            s += -(-int(cnt[rk]) // padto) * padto
        used = -(-s // GROUP) * GROUP
        qid, rank = np.full(ns, 0xFFFFFFFF, _u32), np.zeros(ns, _u32)
        ra, rb = np.zeros(ns, _u32), np.zeros(ns, _u32)
        first = np.concatenate([[0], np.cumsum(cnt)])
        bounds = slot0[1:] + [1 << 40]
        for rk in range(5):
            lo, hi = slot0[rk], min(bounds[rk], ns)
            rank[lo:hi] = rk
            li = f["sorted_idx"][first[rk]:first[rk + 1]].astype(np.int64)
            m = min(len(li), max(0, min(hi, used) - lo))
            li = li[:m]
            qid[lo:lo + m], ra[lo:lo + m], rb[lo:lo + m] = f["qis"][li], f["qa"][li], f["qb"][li]
        lay = np.array(slot0 + [used, slot0[4] if "layout6_in_slots" in rules else slot0[4] // GROUP], _u32)
        return dict(QID=qid, RANK=rank, RA=ra, RB=rb, LAYOUT=lay)

    def inputs(self):
        f0, f1 = self.forms
        return [self.Q, np.array([BATCH_CASE, self.q0, self.nq_range], _u32), self.list, SYN_COUNTS.ravel(),
                f0["sorted_keys"], f0["sorted_idx"], f1["sorted_keys"], f1["sorted_idx"]]

    def with_rules(self, rules):
        return [self._form(f["qis"], rules) for f in self.forms]


_batch = None


def batch():
    global _batch
    if _batch is None:
        _batch = Batch()
    return _batch


# ------------------------------------------------------------------------------------------------------------- blob lists
LAYOUT_GRIDS = ("production", "one", "three")


def out_names():
    """the harness's output blobs, in the order it pushes them"""
    nm = ["SIZES"]
    C = range(len(CASE_N))
    for c in C:
        nm += ["c%d_KEYS_CT" % c, "c%d_KEYS_T" % c, "c%d_IDS" % c]
    for c in C:
        nm += ["c%d_QUANT_plain" % c, "c%d_QUANT_rot" % c]
    for c in C:
        for b in BUILDERS:
            for o in range(2):
                nm += ["c%d_%s_o%d_%s" % (c, b, o, x) for x in ("TILES", "NORMS", "BPOS")]
            nm.append("c%d_%s_BOUNDS" % (c, b))
    for c in C:
        for b in PATCH_FORMATS:
            for p in range(2):
                for o in range(2):
                    nm += ["c%d_%s_patch%d_o%d_%s" % (c, b, p, o, x) for x in ("TILES", "NORMS")]
                nm.append("c%d_%s_patch%d_PATCHED" % (c, b, p))
    for c in C:
        nm += ["c%d_PLAN1" % c, "c%d_PLAN7" % c]
    for f in range(2):
        nm += ["f%d_%s" % (f, x) for x in ("COUNTS", "KEYS", "IDX", "QA", "QB")]
        nm += ["f%d_SYNKEYS%d" % (f, s) for s in range(len(SYN_COUNTS))]
        for g in LAYOUT_GRIDS:
            nm += ["f%d_%s_%s" % (f, g, x) for x in ("QID", "RANK", "RA", "RB", "LAYOUT")]
    for si in range(2):
        for b in BUILDERS:
            for v in range(8):
                nm += ["p%d_%s_v%d_%s" % (si, b, v, x) for x in PREP_FIELDS]
    return nm


def host_names():
    nm = ["SIZES", "CASE_N"]
    for c in range(len(CASE_N)):
        nm += ["c%d_LEVELS" % c, "c%d_BLOCKS" % c]
    return nm + ["KEYS", "KEYS_INV"]


def write_cases(path):
    arrays = []
    for c, fl in zip(cases(), CASE_FLAGS):
        arrays += c.inputs(fl)
    s0, s1 = prep_sets()
    prep = [s0.caps, np.array([s1.c], _u32), s1.Q, s1.caps, np.concatenate([s1.lay[x] for x in ("QID", "RANK", "RA", "RB")])]
    P.write_blobs(path, arrays + batch().inputs() + prep)


def read_results(path, names):
    got = P.read_blobs(path, names)
    return {k: np.asarray(v, _u32) for k, v in got.items()}


# ------------------------------------------------------------------------------------------------------------- the checks
def _exact(what, got, want, describe=None):
    want = np.ascontiguousarray(want).view(_u32).ravel()
    if got.size != want.size:
        return "%s: %d words, the model %d" % (what, got.size, want.size)
    bad = np.nonzero(got != want)[0]
    if bad.size:
        w = int(bad[0])
        return "%s word %d%s: got %#x, model %#x (%d words differ)" % (what, w, " (%s)" % describe(w) if describe else "", int(got[w]),
                                                                      int(want[w]), bad.size)
    return None


def _ulp_up(f):
    return np.nextafter(_f32(f), _f32(np.inf))


class SqrtTally:
    """values behind a device sqrt: how many were compared, how many differed from the model at all"""

    def __init__(self):
        self.compared = self.differed = 0

    def check(self, what, got_bits, model_f32, exact_f64, rel=0.0):
        got = np.array([got_bits], _u32).view(_f32)[0]
        self.compared += 1
        self.differed += int(got != model_f32)
        if not float(got) >= float(exact_f64) * (1.0 - rel):
            return "%s: %r is below the exact value %r" % (what, float(got), float(exact_f64))
        top = _ulp_up(BM.round_up_f32(float(model_f32) * (1.0 + rel))) if rel else _ulp_up(model_f32)
        if not got <= top:
            return "%s: %r is more than one ulp above the model's %r" % (what, float(got), float(model_f32))
        return None


def check_keys(got, rules=frozenset()):
    for c, case in enumerate(cases()):
        kct, ktt, ids = case.keys(rules)[:3]
        lab = lambda w, case=case: "row %d, C %r T %r" % (w // 2, float(case.D[w // 2, 0]), float(case.D[w // 2, 1]))
        for name, want, d in (("KEYS_CT", kct, lab), ("KEYS_T", ktt, lab), ("IDS", ids, None)):
            e = _exact("keys: hvs_k_attr_keys case %s %s" % (case.name, name), got["c%d_%s" % (c, name)], want, d)
            if e:
                return e
    return None


def _one_nan(words):
    """a centre that is NaN (non-finite data) as one bit pattern: which NaN an addition returns is not part of the contract"""
    w = words.copy()
    c = w[:128]
    c[np.isnan(c.view(_f32))] = 0x7FC00000
    return w


def check_quant(got, rules=frozenset()):
    fields = lambda w: ("center[%d]" % w if w < 128 else "sd" if w < 130 else "inv_sd" if w < 132 else "kmin[%d]" % (w - 132) if w < 260
                        else "kmax[%d]" % (w - 260) if w < 388 else "rot")
    for c, case in enumerate(cases()):
        for rot, nm in ((False, "plain"), (True, "rot")):
            e = _exact("quant: case %s %s HvsQuant" % (case.name, nm), _one_nan(got["c%d_QUANT_%s" % (c, nm)][:389]),
                       _one_nan(case.quant(rot, rules).words()[:389]), fields)
            if e:
                return e
    return None


def _check_bounds(tally, what, words, model, exact, rel=0.0):
    for s in range(8):
        name = "%s HvsBounds.%s" % (what, BOUND_NAMES[s])
        if s in SQRT_BOUNDS and np.isfinite(model[s]) and model[s] > 0:
            e = tally.check(name, words[s], model[s], exact[s], rel)
        else:
            e = _exact(name, words[s:s + 1], np.array([model[s]], _f32))
        if e:
            return e
    return None


def _check_norms(what, b, got, m, o):
    """the accumulator inits of the rot builder: floor(v) for some v within 1e-12 of the model's; the others word for word"""
    if b != "rot":
        return _exact(what, got, m.norms[o], lambda w: "storage index %d word %d" % divmod(w, NORM_WORDS[b]))
    want, v = m.norms[o].view(np.int32).astype(np.int64), m.vfloat[o]
    have = got.view(np.int32).astype(np.int64)
    if have.size != want.size:
        return "%s: %d words, the model %d" % (what, have.size, want.size)
    with np.errstate(invalid="ignore"):
        lo, hi = np.floor(v * (1.0 + 1e-12)), np.floor(v * (1.0 - 1e-12))      # v < 0
    ok = np.where(np.isnan(v), have == want, (have >= lo) & (have <= hi))
    bad = np.nonzero(~ok)[0]
    if bad.size:
        w = int(bad[0])
        return "%s storage index %d row %d: got %d, model %d from v = %r" % (what, w // 32, w % 32, have[w], want[w], v[w])
    return None


def near_integer_share(case):
    """share of the rot builder's rows whose un-floored init lies within 1e-12 relative of an integer"""
    v = build_model(case, "rot").vfloat[0]
    v = v[~np.isnan(v)]
    return float(np.mean(np.floor(v * (1.0 + 1e-12)) != np.floor(v * (1.0 - 1e-12)))) if v.size else 0.0


def runs(c, b):
    return bool(CASE_FLAGS[c] & FLAG_TILES) and (b != "f16" or bool(CASE_FLAGS[c] & FLAG_F16))


def check_tiles(got, tally, rules=frozenset()):
    for c, case in enumerate(cases()):
        for b in BUILDERS:
            pre = "c%d_%s" % (c, b)
            if not runs(c, b):
                if got[pre + "_BOUNDS"].size:
                    return "tiles: case %s: builder %s ran" % (case.name, b)
                continue
            m = build_model(case, b, rules)
            for o in range(2):
                what = "tiles: builder %s case %s ordering %d" % (b, case.name, o)
                e = (_exact(what + " blockpos", got["%s_o%d_BPOS" % (pre, o)], m.bpos[o]) or
                     _exact(what + " tile", got["%s_o%d_TILES" % (pre, o)], m.tiles[o], lambda w, b=b: describe_tile_word(b, w)) or
                     _check_norms(what + " norms", b, got["%s_o%d_NORMS" % (pre, o)], m, o))
                if e:
                    return e
            w = got[pre + "_BOUNDS"]
            e = _check_bounds(tally, "tiles: builder %s case %s" % (b, case.name), w, m.bounds, m.exact, 1e-12 if b == "rot" else 0.0)
            if e:
                return e
            if w.size != BOUNDS_WORDS or w[8:13].any():
                return "tiles: builder %s case %s touched the planner's fields of HvsBounds" % (b, case.name)
    return None


def check_patch(got, rules=frozenset()):
    for c, case in enumerate(cases()):
        for b in PATCH_FORMATS:
            if not runs(c, b):
                continue
            m = build_model(case, b, rules, dead=case.dead)
            for p in range(2):
                for o in range(2):
                    what = "patch: format %s case %s ordering %d pass %d" % (b, case.name, o, p)
                    pre = "c%d_%s_patch%d_o%d" % (c, b, p, o)
                    e = (_exact(what + " tile", got[pre + "_TILES"], m.tiles[o], lambda w, b=b: describe_tile_word(b, w)) or
                         _exact(what + " norms", got[pre + "_NORMS"], m.norms[o]))
                    if e:
                        return e
                # both orderings count their dead rows into one counter
                e = _exact("patch: format %s case %s pass %d patched" % (b, case.name, p), got["c%d_%s_patch%d_PATCHED" % (c, b, p)],
                           np.array([2 * int(case.dead.sum())], _u64))
                if e:
                    return e
    return None


def check_plan(got, tally):
    for c, case in enumerate(cases()):
        for step in (1, 7):
            w = got["c%d_PLAN%d" % (c, step)]
            if not CASE_FLAGS[c] & FLAG_TILES:
                continue
            what = "plan: hvs_k_plan_stats case %s step %d" % (case.name, step)
            m = plan_model(case, step)
            if w.size != BOUNDS_WORDS:
                return "%s: %d words" % (what, w.size)
            e = _check_bounds(tally, what, w, m["f"], m["exact"])
            if e:
                return e
            ps, pq = w[8:12].view(_f64)
            if int(w[12]) != m["pair_n"]:
                return "%s pair_n: got %d, model %d" % (what, int(w[12]), m["pair_n"])
            for nm, have, want in (("pair_sum", ps, m["pair_sum"]), ("pair_sumsq", pq, m["pair_sumsq"])):
                if not abs(have - want) <= 1e-12 * abs(want):
                    return "%s %s: got %r, model %r" % (what, nm, float(have), want)
    return None


def check_batch(got, rules=frozenset()):
    B = batch()
    forms = B.with_rules(rules) if rules else B.forms
    for f, fm in enumerate(forms):
        what = "batch: %s form" % ("list" if f else "q0 + range")
        ql = lambda w, fm=fm: "query %d %r" % (fm["qis"][w], B.Q[fm["qis"][w], :4].tolist())
        e = (_exact(what + " hvs_k_count_classes counts", got["f%d_COUNTS" % f], fm["counts"]) or
             _exact(what + " hvs_k_query_keys2 qa", got["f%d_QA" % f], fm["qa"], ql) or
             _exact(what + " hvs_k_query_keys2 qb", got["f%d_QB" % f], fm["qb"], ql) or
             _exact(what + " hvs_k_query_keys2 keys", got["f%d_KEYS" % f], fm["keys"], lambda w: ql(w // 2)) or
             _exact(what + " hvs_k_query_keys2 idx", got["f%d_IDX" % f], fm["idx"]))
        if e:
            return e
        for s in range(len(SYN_COUNTS)):
            e = _exact("%s hvs_k_query_keys2 keys under populations %s" % (what, SYN_COUNTS[s].tolist()), got["f%d_SYNKEYS%d" % (f, s)],
                       B.keys_for(fm, SYN_COUNTS[s]), lambda w: ql(w // 2))
            if e:
                return e
        lay = B.layout(fm, rules)
        for g in LAYOUT_GRIDS:
            for x in ("LAYOUT", "RANK", "QID", "RA", "RB"):
                have = got["f%d_%s_%s" % (f, g, x)]
                have = have[:7] if x == "LAYOUT" else have
                e = _exact("%s hvs_k_layout (%s grid) %s" % (what, g, x.lower()), have, lay[x], (lambda w: "slot %d" % w) if x != "LAYOUT" else None)
                if e:
                    return e
    return None


# ------------------------------------------------------------------------------------------------------------------- prep
PREP_FIELDS = ("RA", "RB", "QN", "NORMQ", "EQ", "NQB", "TOPCNT", "CANDCNT", "OVERFLOW", "TAU", "THETA", "GUA", "GUB", "GORD", "PAIRCNT",
               "GOVERFLOW", "BFRAG", "COUNTERS")
CAP_NOTHING = _f32(-1.0)
EMPTY = 0xFFFFFFFF
DIRTY = 0xEEEEEEEE
CNT_COUNT = 38
# the caps of hvs_k_prep<true>, dealt out query by query: none, "no row is within this cap", 0, a subnormal, one beyond every
# distance (thetai's lower clamp), an ordinary one.  thetai's upper clamp is reached by the |q|^2 = 1e32 query under cap 0.
CAP_CYCLE = np.array([np.inf, -1.0, 0.0, 1.0e-40, 1.0e30, 50.0], _f32)


def variant(v):
    return dict(capped=v >> 2, for_filter=(v >> 1) & 1, count_pairs=v & 1)


class PrepSet:
    def __init__(self, case_index, Q, caps, lay):
        self.c, self.case, self.Q, self.caps, self.lay = case_index, cases()[case_index], Q, caps, lay
        self.nslots = lay["QID"].size
        self.ngroups = self.nslots // GROUP
        self.real = lay["QID"] != EMPTY
        self.qi = np.where(self.real, lay["QID"], 0).astype(np.int64)


_prep_sets = None


def prep_sets():
    """set 0: the range form's layout of the batch section on its case; set 1: one group of type-0 queries on the case whose rows
    are all equal -- scale 1 and a centre on a grid of 1/8, so that components exactly half a step off the grid (the ties of
    rint) exist: query i has every component at centre + (i - 8) + 1/2, query 0 sits on the centre"""
    global _prep_sets
    if _prep_sets is None:
        B = batch()
        f0 = B.forms[0]
        caps0 = CAP_CYCLE[np.arange(B.Q.shape[0]) % CAP_CYCLE.size].copy()
        caps0[B.edge["huge"]] = 0.0
        s0 = PrepSet(BATCH_CASE, B.Q, caps0, B.layout(f0))
        case = cases()[1]
        nq1 = 20
        Q1 = np.zeros((nq1, QCOLS), _f32)
        Q1[:, 4:] = case.V[0][None, :]
        Q1[1:, 4:] += (np.arange(1, nq1) - 8.0 + 0.5).astype(_f32)[:, None]
        Q1[17, 4 + 5] += 300.0                                   # beyond +-127.5: clipped, and far outside a box of width 0
        lay = dict(QID=np.full(GROUP, EMPTY, _u32), RANK=np.zeros(GROUP, _u32), RA=np.zeros(GROUP, _u32), RB=np.zeros(GROUP, _u32))
        lay["QID"][:nq1], lay["RB"][:nq1] = np.arange(nq1), case.n
        s1 = PrepSet(1, Q1, CAP_CYCLE[(np.arange(nq1) + 1) % CAP_CYCLE.size].copy(), lay)
        _prep_sets = [s0, s1]
    return _prep_sets


def _parts_sum(a):
    """hvs_k_prep's sums: "4 lanes, 25 dimensions each, f64 partial sums joined by two shuffles": (p0 + p1) + (p2 + p3)"""
    p = [seq_sum(a[:, 25 * i:25 * i + 25]) for i in range(4)]
    return (p[0] + p[1]) + (p[2] + p[3])


def query_sums(ps, b, rules=frozenset()):
    """per query: qn, e2, nb2, clip, bad, and the image the B fragments are cut from"""
    V = ps.Q[:, 4:]
    with np.errstate(all="ignore"):
        if b in ("bf16", "f16"):
            x = V.astype(_f64)
            bits = h16_bits(b, V)
            xb = h16_val(b, bits).astype(_f64)
            img = np.zeros((V.shape[0], 112), np.uint16)
            img[:, :NDIM] = bits
            img[:, 100:(102 if "bfrag_ones_k_lt_102" in rules else 103)] = 0x3C00 if b == "f16" else 0x3F80
            return dict(qn=_parts_sum(x * x), e2=_parts_sum((x - xb) * (x - xb)), nb2=_parts_sum(xb * xb), clip=np.zeros(V.shape[0]),
                        bad=np.zeros(V.shape[0], bool), img=img)
        qz = ps.case.quant(b == "rot")
        X = rotate_seq(V) if b == "rot" else V.astype(_f64)
        x = X - qz.center[:qz.nd].astype(_f64)
        v = quant_i8(x, qz.inv_sd, rules)
        xq = qz.sd * v
        nan = np.isnan(x)
        inside = np.abs(x * qz.inv_sd) <= 127.5
        d = x - xq
        half = np.roll(qz.half, 1) if "clip_wrong_half" in rules else qz.half
        in_eq = inside | ~nan if "eq_counts_clipped" in rules else inside
        sums = seq_sum if b == "rot" else _parts_sum
        img = np.zeros((V.shape[0], RDIM), np.int8)
        img[:, :qz.nd] = v.astype(np.int64).astype(np.int8)
        return dict(qn=sums(x * x), nb2=sums(xq * xq), e2=sums(np.where(in_eq, d * d, 0.0)),
                    clip=sums(np.where(~inside & ~nan, np.abs(d) * half[None, :] * (1.0 + 1e-9), 0.0)), bad=nan.any(1), img=img)


def _bfrag_map(b, rules=frozenset()):
    """(fragment, lane, element) -> (slot of the group, k), from the comments at the fragment loops of hvs_k_prep"""
    if b in ("bf16", "f16"):     # "lane l of k-step ks holds query column (l & 31), k = 16 ks + 8 (l >> 5) + 0..7"; [qb][ks][lane]
        qb, ks, l, j = np.meshgrid(np.arange(4), np.arange(7), np.arange(64), np.arange(8), indexing="ij")
        return 32 * qb + (l & 31), 16 * ks + 8 * (l >> 5) + j
    if b == "i8":                # "lane l of k-step ks holds query column (l & 31), k = 32 ks + 16 (l >> 5) + 0..15"
        qb, ks, l, j = np.meshgrid(np.arange(4), np.arange(4), np.arange(64), np.arange(16), indexing="ij")
        return 32 * qb + (l & 31), 32 * ks + 16 * (l >> 5) + j
    # "fragment (sub-block j of 16 queries, k-step ks): lane l holds query column 16 j + (l & 15), k = 64 ks + 16 (l >> 4) + 0..15;
    # stored [group][j][ks][lane]"
    if "bfrag_index_swapped" in rules:
        ks, sb, l, j = np.meshgrid(np.arange(2), np.arange(8), np.arange(64), np.arange(16), indexing="ij")
    else:
        sb, ks, l, j = np.meshgrid(np.arange(8), np.arange(2), np.arange(64), np.arange(16), indexing="ij")
    return 16 * sb + (l & 15), 64 * ks + 16 * (l >> (5 if "bfrag_lane_shift5" in rules else 4)) + j


def bfrag_words(ps, b):
    """words hvs_k_prep writes per group, and words of the whole buffer"""
    return (7168 if b in ("bf16", "f16") else 4096), (ps.nslots // 32) * 448 * 4


def theta_i8(qn, normq, eq, nqb, ra, rb, tau, bounds, qz):
    """hvs_theta_i8 on stored f32 / f64 values: +, x, floor and the two clamps"""
    g = 20.0 * 5.9604644775390625e-08
    iu = qz.inv_sd * qz.inv_sd
    with np.errstate(all="ignore"):
        tau = tau.astype(_f64)
        band = (nqb.astype(_f64) * float(bounds[4]) + eq.astype(_f64) * float(bounds[5]) + normq.astype(_f64)) * (1.0 + 1e-6)
        th = (0.5 * (qn * (1.0 - 1e-12) - tau * (1.0 + 2.0 * g)) - band) * iu
        th = np.floor(th - (2.0 + 1e-9 * (qn + tau + band) * iu))
        ti = np.where(th >= 2147483647.0, 0x7FFFFFFF, np.where(th <= -2147483647.0, -0x7FFFFFFF, np.where(np.isnan(th), -0x7FFFFFFF, th)))
    out = np.where(rb > ra, -0x80000000, 0x7FFFFFFF).astype(np.int64)
    return np.where(tau < np.inf, ti.astype(np.int64), out)


def theta_h16(qn, normq, eq, nqb, ra, rb, tau, bounds):
    """hvs_theta_h16: the same, and one f32 round-down"""
    g = 20.0 * 5.9604644775390625e-08
    e_d, nb_d, hmax, rho = (float(bounds[i]) for i in range(4))
    with np.errstate(all="ignore"):
        tau = tau.astype(_f64)
        mu = 256.0 * 5.9604644775390625e-08 * (nqb.astype(_f64) * nb_d + 1.02 * hmax)
        band = mu + rho + normq.astype(_f64) * e_d + eq.astype(_f64) * nb_d
        slack = 1e-9 * (qn + tau + band)
        th = 0.5 * (qn * (1.0 - 1e-12) - tau * (1.0 + 2.0 * g)) - band * (1.0 + 1e-6) - slack
        tf = th.astype(_f32)
        down = np.where(tf == 0, _f32(-1.0e-30), np.nextafter(tf, _f32(-np.inf)))
        tf = np.where(tf.astype(_f64) > th, down, tf).astype(_f32)
    out = np.where(rb > ra, _f32(-np.inf), _f32(np.inf)).astype(_f32)
    return np.where(tau < np.inf, tf, out).astype(_f32)


def _ru_exact(s2, extra=None):
    with np.errstate(invalid="ignore"):
        r = np.sqrt(s2) if extra is None else extra
    return r * (1.0 + 1e-9) + 1e-30


def prep_model(ps, b, v, rules=frozenset(), dev=None):
    """Expected HvsBatch after hvs_k_prep<capped> in format b.  `dev`: the device's own stored qn, normq, eq, nqb and HvsBounds
    (theta / thetai are then the formula on those); None: the model's.  -> {field: words}, and `exact` {field: f64} for the
    values that are rounded up from an f64."""
    V = variant(v)
    fmt_i8 = b in ("i8", "i8x16", "rot")
    qz = ps.case.quant(b == "rot") if fmt_i8 else None
    mb = build_model(ps.case, b)
    bounds = dev["bounds"] if dev else mb.bounds
    qs = query_sums(ps, b, rules)
    real, qi, ns = ps.real, ps.qi, ps.nslots
    pick = lambda a: np.where(real, a[qi], 0.0)
    qn, e2, nb2, clip = pick(qs["qn"]), pick(qs["e2"]), pick(qs["nb2"]), pick(qs["clip"])
    bad = real & qs["bad"][qi]
    a0, b0 = ps.lay["RA"].astype(np.int64), ps.lay["RB"].astype(np.int64)
    with np.errstate(all="ignore"):
        hopeless = bad.copy()
        if fmt_i8:
            rest = np.sqrt(nb2) * float(bounds[4]) + np.sqrt(e2) * float(bounds[5])
            hopeless |= real & ~(clip <= (2.0 if "hopeless_2x" in rules else 4.0) * rest)
        elif b == "f16":
            if "f16_flush_left_out" not in rules:
                r = np.sqrt(e2) + BM.F16_FLUSH
                e2 = np.where(real, r * r, e2)
            hopeless |= real & ~(nb2 < 1.0e9)
        hopeless |= ~(qn < 1.0e30)
        hopeless &= real & bool(V["for_filter"])
        pairs = int(np.where(real & (b0 > a0), b0 - a0, 0).sum()) if V["count_pairs"] else 0
        ra, rb = np.where(hopeless, 0, a0), np.where(hopeless, 0, b0)
        ex = dict(EQ=_ru_exact(e2), NQB=_ru_exact(nb2))
        if fmt_i8:
            ex["NORMQ"] = clip
            normq = np.where(clip > 0.0, BM.round_up_f32(np.where(clip > 0.0, clip, 1.0)), _f32(0)).astype(_f32)
        else:
            ex["NORMQ"] = _ru_exact(qn)
            normq = BM.round_up_f32(ex["NORMQ"])
        eq, nqb = BM.round_up_f32(ex["EQ"]), BM.round_up_f32(ex["NQB"])
    caps = np.where(real, ps.caps[qi], _f32(np.inf)).astype(_f32)
    tau = caps if V["capped"] else np.full(ns, np.inf, _f32)
    s_qn, s_normq, s_eq, s_nqb = (dev["QN"], dev["NORMQ"], dev["EQ"], dev["NQB"]) if dev else (qn, normq, eq, nqb)
    if "theta_from_wrong_norm" in rules:
        s_normq = s_nqb
    if V["capped"]:
        t_tau = np.full(ns, np.inf, _f32) if "capped_theta_from_inf" in rules else tau
        nothing = (caps == CAP_NOTHING) & ("cap_nothing_keeps_all" not in rules)
        if fmt_i8:
            th = np.where(nothing, 0x7FFFFFFF, theta_i8(s_qn, s_normq, s_eq, s_nqb, ra, rb, t_tau, bounds, qz))
        else:
            th = np.where(nothing, _f32(np.inf), theta_h16(s_qn, s_normq, s_eq, s_nqb, ra, rb, t_tau, bounds)).astype(_f32)
    elif fmt_i8:
        th = np.where(rb > ra, -0x80000000, 0x7FFFFFFF)
    else:
        th = np.where(rb > ra, _f32(-np.inf), _f32(np.inf)).astype(_f32)
    theta = th.astype(np.int64).astype(np.int32).view(_u32) if fmt_i8 else th.view(_u32)
    # per group: "union of the slots' ranges, ordering, cleared entry counters"
    A, Bb = ra.reshape(-1, GROUP), rb.reshape(-1, GROUP)
    use = A < Bb
    gua = np.where(use, A, 1 << 40).min(1)
    gub = np.where(use, Bb, 0).max(1)
    anyu = use.any(1)
    gord = (ps.lay["RANK"].reshape(-1, GROUP)[:, 0] == 4).astype(_u32)
    # the B fragments: a padding slot's column is zero
    img = np.where(real[:, None], qs["img"][qi], 0).astype(qs["img"].dtype)
    slot, k = _bfrag_map(b, rules)
    fr = img.reshape(ps.ngroups, GROUP, -1)[:, slot, k]
    per, total = bfrag_words(ps, b)
    bfrag = np.full(total, DIRTY, _u32)
    bfrag[:per * ps.ngroups] = np.ascontiguousarray(fr).view(_u32).ravel()
    counters = np.zeros(CNT_COUNT, _u64)
    counters[0] = pairs
    zs, zg = np.zeros(ns, _u32), np.zeros(ps.ngroups, _u32)
    out = dict(RA=ra.astype(_u32), RB=rb.astype(_u32), QN=qn, NORMQ=normq, EQ=eq, NQB=nqb, TOPCNT=zs, CANDCNT=zs, OVERFLOW=np.where(hopeless, 2, 0).astype(_u32),
               TAU=tau, THETA=theta, GUA=np.where(anyu, gua, 0).astype(_u32), GUB=np.where(anyu, gub, 0).astype(_u32), GORD=gord, PAIRCNT=zg,
               GOVERFLOW=zg, BFRAG=bfrag, COUNTERS=counters)
    return out, ex, dict(clip=clip, rest=rest if fmt_i8 else None, hopeless=hopeless)


def describe_bfrag_word(b, w):
    per = 7168 if b in ("bf16", "f16") else 4096
    g, r = divmod(int(w), per)
    slot, k = _bfrag_map(b)
    el = 8 if b in ("bf16", "f16") else 16
    frag, r = divmod(r, 256)
    lane, p = divmod(r, 4)
    j0 = p * el // 4
    s2, k2 = slot.reshape(-1, 64, el), k.reshape(-1, 64, el)
    if frag >= s2.shape[0]:
        return "behind the fragments"
    return "group %d fragment %d lane %d word %d = slot %d, k %d.." % (g, frag, lane, p, g * GROUP + s2[frag, lane, j0], k2[frag, lane, j0])


def _same_or_nan32(got, want):
    g, w = got.view(_f32), np.ascontiguousarray(want, _f32)
    return (got == w.view(_u32)) | (np.isnan(g) & np.isnan(w))


def _check_rounded_up(tally, what, got, model, exact, rel):
    """f32 values rounded up from an f64 (behind a device sqrt, or an order-dependent sum when rel > 0): at or above the exact
    value, at most one ulp above the model's; NaN where the model is NaN"""
    g = got.view(_f32)
    model = np.ascontiguousarray(model, _f32)
    with np.errstate(all="ignore"):
        nan = np.isnan(model)
        top = np.nextafter(BM.round_up_f32(np.where(nan | (model <= 0), 1.0, model.astype(_f64) * (1.0 + rel))), _f32(np.inf)) if rel else \
            np.nextafter(model, _f32(np.inf))
        ok = np.where(nan, np.isnan(g), np.where(model == 0, g == 0, (g.astype(_f64) >= exact * (1.0 - rel)) & (g <= top)))
    tally.compared += int(g.size)
    tally.differed += int((~_same_or_nan32(got, model)).sum())
    bad = np.nonzero(~ok)[0]
    if bad.size:
        w = int(bad[0])
        return "%s slot %d: got %r, model %r from the exact %r (%d slots)" % (what, w, float(g[w]), float(model[w]), float(exact[w]), bad.size)
    return None


def check_prep(got, tally, rules=frozenset()):
    for si, ps in enumerate(prep_sets()):
        for b in BUILDERS:
            bounds = got["c%d_%s_BOUNDS" % (ps.c, b)].view(_f32)[:8]
            for v in range(8):
                pre = "p%d_%s_v%d_" % (si, b, v)
                what = "prep: set %d hvs_k_prep<%s> format %s for_filter %d count_pairs %d" % (si, "true" if v >> 2 else "false", b, (v >> 1) & 1, v & 1)
                dev = dict(bounds=bounds, QN=got[pre + "QN"].view(_f64), NORMQ=got[pre + "NORMQ"].view(_f32), EQ=got[pre + "EQ"].view(_f32),
                           NQB=got[pre + "NQB"].view(_f32))
                m, ex, _ = prep_model(ps, b, v, rules, dev)
                rel = 1e-12 if b == "rot" else 0.0
                for f in ("RA", "RB", "TOPCNT", "CANDCNT", "OVERFLOW", "GUA", "GUB", "GORD", "PAIRCNT", "GOVERFLOW", "COUNTERS"):
                    e = _exact("%s %s" % (what, f.lower()), got[pre + f], m[f], (lambda w: "slot %d" % w) if m[f].size == ps.nslots else None)
                    if e:
                        return e
                e = _exact(what + " bfrag", got[pre + "BFRAG"], m["BFRAG"], lambda w, b=b: describe_bfrag_word(b, w))
                if e:
                    return e
                for f in ("TAU", "THETA"):
                    ok = _same_or_nan32(got[pre + f], m[f].view(_f32)) if (f == "TAU" or b in ("bf16", "f16")) else got[pre + f] == m[f]
                    if not ok.all():
                        w = int(np.nonzero(~ok)[0][0])
                        return "%s %s slot %d (query %d): got %#x, model %#x from the device's own norms (%d slots)" % (
                            what, f.lower(), w, int(ps.lay["QID"][w]), int(got[pre + f][w]), int(m[f].view(_u32)[w]), int((~ok).sum()))
                gq, mq = got[pre + "QN"].view(_f64), m["QN"]
                with np.errstate(invalid="ignore"):
                    ok = (np.isnan(gq) & np.isnan(mq)) | (np.abs(gq - mq) <= rel * np.abs(mq))
                if not ok.all():
                    w = int(np.nonzero(~ok)[0][0])
                    return "%s qn slot %d: got %r, model %r" % (what, w, float(gq[w]), float(mq[w]))
                for f in ("EQ", "NQB", "NORMQ"):
                    if f == "NORMQ" and b in ("i8", "i8x16"):      # the clip term: a fixed-order sum, no sqrt
                        ok = _same_or_nan32(got[pre + f], m[f])
                        e = None if ok.all() else "%s normq slot %d: got %#x, model %#x" % (what, int(np.nonzero(~ok)[0][0]), 0, 0)
                    else:
                        e = _check_rounded_up(tally, "%s %s" % (what, f.lower()), got[pre + f], m[f], ex[f], rel)
                    if e:
                        return e
    return None


def _decode_tiles(got, c, b, L, K, dt):
    """the device's tiles of ordering 0 as [valid position, K] in position order, with the row ids"""
    case = cases()[c]
    row, k = tile_map(b)
    t = got["c%d_%s_o0_TILES" % (c, b)].view(dt).reshape((L.nblk,) + row.shape)
    img = np.zeros((L.nblk, 32, K), dt)
    img[:, row, k] = t
    pos = L.blocks[:, None] * 32 + np.arange(32)[None, :]
    valid = pos < case.n
    return img[valid], case.perm[0][pos[valid]], valid


def _decode_bfrag(got, ps, si, b, K, dt):
    slot, k = _bfrag_map(b)
    per, _ = bfrag_words(ps, b)
    fr = got["p%d_%s_v2_BFRAG" % (si, b)][:per * ps.ngroups].view(dt).reshape((ps.ngroups,) + slot.shape)
    img = np.zeros((ps.ngroups, GROUP, K), dt)
    img[:, slot, k] = fr
    return img.reshape(ps.nslots, K)


def cross_check(got):
    """The closing check, on the batch section's case (n = 4100) and the range form's queries with finite components: from the
    device's I8X16 tiles, norms and B fragments, decoded by the layout maps, S = qq.dq + nh in integers for every (query, row)
    must be tests/bound_model.py's S; the decoded BF16 and F16 operands (rows with their three pieces, queries with their ones)
    must give its `est` within the f64 summation bound.  Shows that the builders and hvs_k_prep fill the maps consistently."""
    ps, si = prep_sets()[0], 0
    case, L = ps.case, levels(ps.case.n)
    slots = np.nonzero(ps.real & np.isfinite(ps.Q[ps.qi, 4:]).all(1))[0]
    q = ps.Q[ps.qi[slots], 4:]
    with np.errstate(all="ignore"):
        ref = BM._int8_model(case.V.astype(_f64), q.astype(_f64), False)[3]
    d8, rid, valid = _decode_tiles(got, ps.c, "i8x16", L, RDIM, np.int8)
    nh = got["c%d_i8x16_o0_NORMS" % ps.c].view(np.int32).reshape(L.nblk, 32)[valid].astype(_f64)
    q8 = _decode_bfrag(got, ps, si, "i8x16", RDIM, np.int8)[slots]
    S = q8.astype(_f64) @ d8.astype(_f64).T + nh[None, :]
    want = ref["qq"] @ ref["dq"][rid].T + ref["nh"][rid][None, :]
    bad = np.argwhere(S != want)
    if bad.size:
        return "cross-check: I8X16 query %d row %d: S %r, bound_model %r (%d pairs)" % (
            int(ps.lay["QID"][slots[bad[0][0]]]), int(rid[bad[0][1]]), S[tuple(bad[0])], want[tuple(bad[0])], len(bad))
    for b, fm in (("bf16", BM.BF16), ("f16", BM.FP16)):
        with np.errstate(all="ignore"):
            ref = BM._h16_model(fm, case.V, q)
            d16, rid, _ = _decode_tiles(got, ps.c, b, L, 112, np.uint16)
            q16 = _decode_bfrag(got, ps, si, b, 112, np.uint16)[slots]
            dv, qv = h16_val(b, d16).astype(_f64), h16_val(b, q16).astype(_f64)
            fin = np.isfinite(qv).all(1)
            est, want = qv[fin] @ dv.T, ref[1][fin][:, rid]
            bad = np.argwhere(~(np.abs(est - want) <= 1e-12 * (np.abs(qv[fin]) @ np.abs(dv).T)))
        if bad.size:
            return "cross-check: %s query slot %d row %d: est %r, bound_model %r (%d pairs)" % (
                b, int(slots[fin][bad[0][0]]), int(rid[bad[0][1]]), est[tuple(bad[0])], want[tuple(bad[0])], len(bad))
    return None


# ---------------------------------------------------------------------------------------------------------- the harness
def build_harness(exe):
    """tests/device_index.hip -> exe with the engine's own flags; returns the compile's wall time in seconds"""
    t0 = time.time()
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + P.harness_flags() +
                       [os.path.join(T.REPO, "tests", "device_index.hip"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return time.time() - t0
