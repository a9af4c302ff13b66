"""An f64 model of the filter bounds and adversarial data sets that make them tight.

The filter engines drop a (query, row) pair when the matrix-core estimate S lies below theta (`hvs_k_merge`,
csrc/hvs_filter.h); theta is built from a band of error terms.  This module recomputes, the way the device does, every
quantity the band is made of -- per-dimension box and centre, scale, rounded images, row maxima rounded up to f32, query
norms -- and returns for every (query, row) pair

    lhs       the real-arithmetic side, (|q'|^2 - T) / 2 with T = |q - d|^2 of the f32 inputs
              (= q'.d' - |d'|^2/2 for the INT8 formats, q.d - |d|^2/2 for the 16-bit float ones)
    est       the estimate side: sd^2 (S + 1) (INT8; S = qq.dq + nh, exact on the device) or
              q~.d~ + h0 + h1 + h2 (BF16 / FP16; the device adds an accumulation error, mu)
    terms     each band term separately: "E_D", "e_q", "clip" (INT8), "rho", "mu" (16-bit float formats)

so that the bound reads  lhs <= est + sum(terms)  and a pair uses the fraction (lhs - est) / band of it.

The generators build data on which that fraction comes close to 1 for rows placed in a query's true top-k, with k decoy
rows just behind them: a band that is a little too small then drops a true neighbour and changes the answer
(tests/test_filter_bounds.py runs them through the production library and through mutant builds with a smaller band).
"""
from __future__ import annotations

import numpy as np

NDIM, RDIM = 100, 128
DCOLS, QCOLS = 102, 104
F16_FLUSH = 6.103515625e-4        # HVS_F16_FLUSH: sqrt(100) 2^-14 on every FP16 error norm
F16_FLUSH_RHO = 1.8310546875e-4   # HVS_F16_FLUSH_RHO: 3 x 2^-14 on rho
MU_UNIT = 256.0 * 5.9604644775390625e-08

PLAIN_I8, ROT_I8, BF16, FP16 = "i8", "i8_rot", "bf16", "f16"


# --------------------------------------------------------------------------- f32 helpers (the device's roundings)

def round_up_f32(x):
    """hvs_round_up_f32: the f32 at or above x (x > 0)."""
    x = np.asarray(x, np.float64)
    f = x.astype(np.float32)
    up = f.astype(np.float64) < x
    return np.where(up, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)


def _f32_below(y):
    f = y.astype(np.float32)
    return np.where(f.astype(np.float64) > y, np.nextafter(f, np.float32(-np.inf)), f)


def _f32_above(y):
    f = y.astype(np.float32)
    return np.where(f.astype(np.float64) < y, np.nextafter(f, np.float32(np.inf)), f)


def bf16_round(x):
    """hvs_bf16_bits -> f32: round to nearest even on the top 16 bits."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    return (b.astype(np.uint32) << 16).view(np.float32)


def f16_round(x):
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def _h16(fmt, x):
    return f16_round(x) if fmt == FP16 else bf16_round(x)


# --------------------------------------------------------------------------- the rotation of §3.2a

def rot_signs():
    """hvs_rot_sign(j) for the 100 input dimensions."""
    j = np.arange(NDIM, dtype=np.uint64)
    return ((((j + 1) * 0x9E3779B1) & 0xFFFFFFFF) >> 17) & 1


def rot_matrix():
    """R[k, j] = +-1: hvs_rot_elem(x, k) = sum_j R[k, j] x_j / sqrt(128)."""
    k = np.arange(RDIM)[:, None]
    j = np.arange(NDIM)[None, :]
    pc = np.vectorize(lambda v: bin(int(v)).count("1"))(k & j)
    return np.where(((pc + rot_signs()[None, :].astype(np.int64)) & 1) != 0, -1.0, 1.0)


_R = None


def rotate(x):
    """y = H S pad(x) / sqrt(128) in f64 (the device's hvs_rot_elem; 1/sqrt(128) as the same double constant)."""
    global _R
    if _R is None:
        _R = rot_matrix()
    return (np.asarray(x, np.float64) @ _R.T) * 0.08838834764831844055


# --------------------------------------------------------------------------- the model

def _split(nodes, queries):
    nodes = np.ascontiguousarray(nodes, np.float32)
    queries = np.ascontiguousarray(queries, np.float32)
    assert nodes.shape[1] == DCOLS and queries.shape[1] == QCOLS
    return nodes[:, 2:], queries[:, 4:]


def _true_dist(d, q):
    """T = |q - d|^2 of the f32 inputs, in f64 (relative error ~1e-16): [nq, n]."""
    d64, q64 = d.astype(np.float64), q.astype(np.float64)
    return np.maximum((q64 * q64).sum(1)[:, None] + (d64 * d64).sum(1)[None, :] - 2.0 * q64 @ d64.T, 0.0)


def _int8_model(dv, qv, rotated):
    """dv, qv: [n, m] / [nq, m] f64 vectors in the space the tiles are cut from (m = 100, or 128 rotated)."""
    if rotated:   # hvs_k_minmax_rot: f32 min / max of the f64 components, rounded outward
        lo_f, hi_f = _f32_below(dv).min(0), _f32_above(dv).max(0)
    else:         # hvs_k_minmax: of the f32 components themselves
        lo_f, hi_f = dv.min(0), dv.max(0)
    lo, hi = lo_f.astype(np.float64), hi_f.astype(np.float64)
    c = (0.5 * (lo + hi)).astype(np.float32).astype(np.float64)   # hvs_k_quant_params: f32 midrange
    half = np.maximum(np.abs(lo - c), np.abs(hi - c))
    m = half.max()
    sd = m / 127.0 * (1.0 + 1e-9) if m > 0.0 else 1.0
    inv_sd = 1.0 / sd
    x = dv - c
    dq = np.clip(np.rint(x * inv_sd), -127, 127)
    nd = (x * x).sum(1)
    e2 = ((x - sd * dq) ** 2).sum(1)
    nh = np.floor(-0.5 * nd * inv_sd * inv_sd)
    e_d8 = round_up_f32(np.sqrt(e2) * (1.0 + 1e-9) + 1e-30).max()
    n_d8 = round_up_f32(np.sqrt(nd) * (1.0 + 1e-9) + 1e-30).max()
    xq_ = qv - c
    qq = np.clip(np.rint(xq_ * inv_sd), -127, 127)
    xq = sd * qq
    qn = (xq_ * xq_).sum(1)
    nb2 = (xq * xq).sum(1)
    inside = np.abs(xq_ * inv_sd) <= 127.5
    e2q = np.where(inside, (xq_ - xq) ** 2, 0.0).sum(1)
    clip = np.where(inside, 0.0, np.abs(xq_ - xq) * half[None, :] * (1.0 + 1e-9)).sum(1)
    normq = np.where(clip > 0.0, round_up_f32(np.where(clip > 0.0, clip, 1.0)), np.float32(0.0)).astype(np.float64)
    eq = round_up_f32(np.sqrt(e2q) * (1.0 + 1e-9) + 1e-30).astype(np.float64)
    nqb = round_up_f32(np.sqrt(nb2) * (1.0 + 1e-9) + 1e-30).astype(np.float64)
    S = qq @ dq.T + nh[None, :]                            # exact: |qq.dq| <= 128 * 127^2 < 2^53
    est = sd * sd * (S + 1.0)
    nq, n = qv.shape[0], dv.shape[0]
    terms = {"E_D": np.broadcast_to((nqb * float(e_d8))[:, None], (nq, n)),
             "e_q": np.broadcast_to((eq * float(n_d8))[:, None], (nq, n)),
             "clip": np.broadcast_to(normq[:, None], (nq, n))}
    rest = np.sqrt(nb2) * float(e_d8) + np.sqrt(e2q) * float(n_d8)
    info = dict(sd=sd, center=c, half=half, e_d8=float(e_d8), n_d8=float(n_d8), qn=qn, eq=eq, nqb=nqb, clip=normq,
                hopeless=~(clip <= 4.0 * rest), dq=dq, qq=qq, nh=nh)
    return qn, est, terms, info


def _h16_model(fmt, d, q):
    d64, q64 = d.astype(np.float64), q.astype(np.float64)
    db = _h16(fmt, d).astype(np.float64)
    qb = _h16(fmt, q).astype(np.float64)
    flush, flush_rho = (F16_FLUSH, F16_FLUSH_RHO) if fmt == FP16 else (0.0, 0.0)
    nd = (d64 * d64).sum(1)
    e2 = ((d64 - db) ** 2).sum(1)
    nb2 = (db * db).sum(1)
    # -|d|^2/2 as three 16-bit pieces (hvs_k_build_tiles; the remainders in f32 arithmetic)
    hf = (-0.5 * nd).astype(np.float32)
    h0 = _h16(fmt, hf)
    r1 = (hf - h0).astype(np.float32)
    h1 = _h16(fmt, r1)
    r2 = (r1 - h1).astype(np.float32)
    h2 = _h16(fmt, r2)
    hs = h0.astype(np.float64) + h1.astype(np.float64) + h2.astype(np.float64)
    e_d = float(round_up_f32(np.sqrt(e2) + flush).max())
    nb_d = float(round_up_f32(np.sqrt(nb2)).max())
    hmax = float(round_up_f32(0.5 * nd).max())
    rho = float(round_up_f32(np.abs(0.5 * nd + hs) + flush_rho + 1e-30).max())
    qn = (q64 * q64).sum(1)
    e2q = ((q64 - qb) ** 2).sum(1)
    if fmt == FP16:
        e2q = (np.sqrt(e2q) + F16_FLUSH) ** 2
    nb2q = (qb * qb).sum(1)
    normq = round_up_f32(np.sqrt(qn) * (1.0 + 1e-9) + 1e-30).astype(np.float64)
    eq = round_up_f32(np.sqrt(e2q) * (1.0 + 1e-9) + 1e-30).astype(np.float64)
    nqb = round_up_f32(np.sqrt(nb2q) * (1.0 + 1e-9) + 1e-30).astype(np.float64)
    est = qb @ db.T + hs[None, :]
    mu = MU_UNIT * (nqb * nb_d + 1.02 * hmax)
    nq, n = q.shape[0], d.shape[0]
    terms = {"E_D": np.broadcast_to((normq * e_d)[:, None], (nq, n)),
             "e_q": np.broadcast_to((eq * nb_d)[:, None], (nq, n)),
             "rho": np.full((nq, n), rho),
             "mu": np.broadcast_to(mu[:, None], (nq, n))}
    info = dict(e_d=e_d, nb_d=nb_d, hmax=hmax, rho=rho, qn=qn, normq=normq, eq=eq, nqb=nqb, mu=mu)
    return qn, est, terms, info


def bound_model(fmt, nodes, queries):
    """The bound of format `fmt` (PLAIN_I8, ROT_I8, BF16, FP16) for every (query, row) pair of the data set.

    Returns a dict: lhs, est [nq, n]; terms {name: [nq, n]}; band = sum of the terms; used = (lhs - est) / band;
    slack = est + band - lhs (>= 0 where the bound holds); info (the device-side quantities)."""
    d, q = _split(nodes, queries)
    T = _true_dist(d, q)
    if fmt == PLAIN_I8:
        qn, est, terms, info = _int8_model(d.astype(np.float64), q.astype(np.float64), False)
    elif fmt == ROT_I8:
        qn, est, terms, info = _int8_model(rotate(d), rotate(q), True)
    elif fmt in (BF16, FP16):
        qn, est, terms, info = _h16_model(fmt, d, q)
    else:
        raise ValueError(fmt)
    lhs = 0.5 * (qn[:, None] - T)
    band = sum(terms.values())
    return dict(lhs=lhs, est=est, terms=terms, band=band, used=(lhs - est) / band, slack=est + band - lhs, T=T,
                qn=qn, info=info)


def bound_holds(m, rtol=1e-9):
    """Every pair satisfies lhs <= est + band up to a relative tolerance of the magnitudes involved (the f64 evaluation)."""
    scale = np.abs(m["qn"])[:, None] + np.abs(m["T"]) + np.abs(m["band"]) + np.abs(m["est"])
    return m["slack"] >= -rtol * scale


# --------------------------------------------------------------------------- adversarial data sets

class AdvSet:
    """nodes [n, 102] and queries [nq, 104] (f32), the format the set was built for, the terms it loads, and per query the row
    id of its built-for row (`tight`; the nearest row its predicate admits) and the fraction of the band that row must use."""

    def __init__(self, name, fmt, nodes, queries, tight, target, terms):
        self.name, self.fmt, self.nodes, self.queries = name, fmt, nodes, queries
        self.tight, self.target, self.terms = tight, target, terms


def _assemble(name, fmt, groups, extra_rows, nq, rng, target, terms, qtypes, vecq):
    """groups[i]: list of (vector, cat, time) for query i, its tight row first; extra_rows: (vector, cat, time) of no query."""
    rows, owner, is_tight = [], [], []
    for i, g in enumerate(groups):
        for j, (v, c, t) in enumerate(g):
            rows.append((v, c, t))
            owner.append(i)
            is_tight.append(j == 0)
    for r in extra_rows:
        rows.append(r)
        owner.append(-1)
        is_tight.append(False)
    perm = rng.permutation(len(rows))
    nodes = np.zeros((len(rows), DCOLS), np.float32)
    tight = np.full(nq, -1, np.int64)
    for new, old in enumerate(perm):
        v, c, t = rows[old]
        nodes[new, 0], nodes[new, 1], nodes[new, 2:] = c, t, v
        if is_tight[old]:
            tight[owner[old]] = new
    queries = np.zeros((nq, QCOLS), np.float32)
    for i in range(nq):
        typ = qtypes[i]
        queries[i, 0] = typ
        queries[i, 1:4] = (i, 0.0, 1000.0) if typ == 3 else (-1.0, -1.0, -1.0)
        queries[i, 4:] = vecq[i]
    return AdvSet(name, fmt, nodes, queries, tight, target, terms)


def _grid_group(sigma, lo_dims, u, lo, m_range, ndecoy, rng, cat, fixed=None):
    """Rows of one query on an 8-bit-style grid of unit u (see int8_set).  In the dimensions `lo_dims` the tight row sits at
    (lo + 0.4999) u, the decoys at lo u or (lo + 1) u -- m of them at lo + 1, so their distance lies just above the tight row's;
    `fixed` (dimensions, value) pins other dimensions of every row of the group to one on-grid value."""
    free = np.nonzero(lo_dims)[0]
    tight = np.zeros(NDIM)
    tight[free] = lo + 0.4999
    if fixed is not None:
        tight[fixed[0]] = fixed[1]
    group = [((sigma * tight * u).astype(np.float32), cat, float(rng.uniform(0, 1000)))]
    for _ in range(ndecoy):
        m = int(rng.integers(m_range[0], m_range[1] + 1))
        v = np.zeros(NDIM)
        v[free] = lo
        v[rng.choice(free, m, replace=False)] = lo + 1
        if fixed is not None:
            v[fixed[0]] = fixed[1]
        group.append(((sigma * v * u).astype(np.float32), cat, float(rng.uniform(0, 1000))))
    return group


def _decoy_m(nfree, a, lo_off):
    """Smallest m with  (nfree - m) (lo - a)^2 + m (lo + 1 - a)^2  >  nfree (lo + 0.4999 - a)^2  (distances in grid units)."""
    t = nfree * (lo_off + 0.4999 - a) ** 2
    base = nfree * (lo_off - a) ** 2
    step = (lo_off + 1 - a) ** 2 - (lo_off - a) ** 2
    return int(np.floor((t - base) / step)) + 1


def int8_set(seed=11, nq=64, ndecoy=500, clipped=False, type3=True):
    """Plain INT8, grid unit u = 1/8: two corner rows at +-127 u fix the centre at 0 and sd = u (1 + 1e-9).  Query i
    has a random sign vector sigma; its tight row A = sigma 126.4999 u rounds to 126 with an error of 0.4999 u parallel to
    qq = sigma 100 (the query sigma 100.4999 u); the query's rounding error 0.4999 u sigma is parallel to A itself.  Both
    Cauchy-Schwarz steps of the band are then nearly equalities -- A uses 0.998 of it, the E_D term carries 44 %, the e_q term
    56 %.  Its decoys (on the grid, no rounding error) sit at distances just above A's, so A is the nearest row and a band a few
    per cent too small drops it from the answer.

    `clipped` (set b): 20 dimensions of every query lie 4.5 u beyond the box (127.5 + 4 units); A and its decoys sit on the box
    edge there (sigma 127 u), so the clip term sum_k c_k H_k is exact for A.  It carries about half of the band and stays
    below 4x the rest (no query goes to the exact engine).

    `type3`: every other query is a type-3 query (its own category, times [0, 1000]); 16 rows of that category at the query's
    own grid point but a later time must stay out of its answer."""
    rng = np.random.default_rng(seed)
    u = 0.125
    groups, vecq, qtypes, extra = [], [], [], []
    for i in range(nq):
        sigma = rng.choice([-1.0, 1.0], NDIM)
        qv = np.full(NDIM, 100.4999)
        lo_dims = np.ones(NDIM, bool)
        fixed = None
        if clipped:
            cd = rng.choice(NDIM, 20, replace=False)
            lo_dims[cd] = False
            qv[cd] = 127.5 + 4.0
            fixed = (cd, 127.0)
        nfree = int(lo_dims.sum())
        m0 = _decoy_m(nfree, 100.4999, 126)
        g = _grid_group(sigma, lo_dims, u, 126, (m0, m0 + 6), ndecoy, rng, float(i), fixed)
        groups.append(g)
        vecq.append((sigma * qv * u).astype(np.float32))
        typ = 3 if (type3 and i % 2 == 1) else 0
        qtypes.append(typ)
        if typ == 3:
            for _ in range(16):
                extra.append(((sigma * 101.0 * u).astype(np.float32), float(i), 5000.0))
    for s in (1.0, -1.0):
        extra.append((np.full(NDIM, s * 127.0 * u, np.float32), 1.0e6, 0.0))
    if clipped:
        return _assemble("b_int8_clipped", PLAIN_I8, groups, extra, nq, rng, 0.93, ("E_D", "e_q", "clip"), qtypes, vecq)
    return _assemble("a_int8", PLAIN_I8, groups, extra, nq, rng, 0.99, ("E_D", "e_q"), qtypes, vecq)


def rotated_set(seed=13, nq=64, ndecoy=500):
    """Rotated INT8, built in y-space.  A spike x = v e_j maps to y = v / sqrt(128) W_j, W_j the Walsh sign pattern
    of input dimension j (every |y_k| equal): query i uses spike j = i, so its tight row (y = 126.4999 u W_j), its query
    (y = 100.4999 u W_j) and their rounding errors are all parallel, as in the plain set.  Rows +-127 u W_99 fix the rotated box
    (centre 0, sd = u); decoys 74 u W_j + sum of p unit spikes of other patterns (p <= 20: |y_k| <= 94 u) lie on the grid at
    (26.5^2 + p) 128 u^2, inside the window a band of half the size opens (A itself at 26^2 128 u^2)."""
    assert nq <= 99
    rng = np.random.default_rng(seed)
    u = 0.125
    s = np.sqrt(128.0) * u
    groups, vecq, qtypes, extra = [], [], [], []

    def spike(j, v):
        x = np.zeros(NDIM)
        x[j] = v * s
        return x
    for i in range(nq):
        g = [(spike(i, 126.4999).astype(np.float32), float(i), float(rng.uniform(0, 1000)))]
        others = np.array([j for j in range(NDIM - 1) if j != i])
        for _ in range(ndecoy):
            x = spike(i, 74.0)
            p = int(rng.integers(0, 21))
            x[rng.choice(others, p, replace=False)] = rng.choice([-1.0, 1.0], p) * s
            g.append((x.astype(np.float32), float(i), float(rng.uniform(0, 1000))))
        groups.append(g)
        vecq.append(spike(i, 100.4999).astype(np.float32))
        qtypes.append(0)
    for sg in (1.0, -1.0):
        extra.append((spike(NDIM - 1, sg * 127.0).astype(np.float32), 1.0e6, 0.0))
    return _assemble("c_int8_rotated", ROT_I8, groups, extra, nq, rng, 0.5, ("E_D", "e_q"), qtypes, vecq)


def float_set(fmt, seed=17, nq=64, ndecoy=500):
    """BF16 or FP16 (§3.3): the same construction on the 16-bit float grid of [8, 16) (ulp 2^-4 / 2^-7): the tight
    row sigma (12 + 0.4999 ulp) and the query sigma (10 + 0.4999 ulp) are nearly half an ulp off the grid with aligned signs,
    decoys mix 12 and 12 + ulp.  At these magnitudes the rounding error (0.039 in FP16) dominates the flush allowance
    HVS_F16_FLUSH (0.0006); rho stays below 10^-3 of the band, mu at 3 % (FP16) / 0.4 % (BF16)."""
    rng = np.random.default_rng(seed)
    ulp = 2.0 ** -4 if fmt == BF16 else 2.0 ** -7
    groups, vecq, qtypes = [], [], []
    for i in range(nq):
        sigma = rng.choice([-1.0, 1.0], NDIM)
        # in units of ulp: tight row 12/ulp + 0.4999, decoys 12/ulp (+1), query 10/ulp + 0.4999
        lo = 12.0 / ulp
        m0 = _decoy_m(NDIM, 10.0 / ulp + 0.4999, lo)
        g = _grid_group(sigma, np.ones(NDIM, bool), ulp, lo, (m0 + 1, m0 + 8), ndecoy, rng, float(i))
        groups.append(g)
        vecq.append((sigma * (10.0 + 0.4999 * ulp)).astype(np.float32))
        qtypes.append(3 if i % 4 == 3 else 0)
    name = "e_bf16" if fmt == BF16 else "d_f16"
    return _assemble(name, fmt, groups, [], nq, rng, 0.9, ("E_D", "e_q"), qtypes, vecq)


def all_sets():
    return [int8_set(), int8_set(seed=12, clipped=True, type3=False), rotated_set(), float_set(FP16), float_set(BF16)]


def used_of_band(m, adv, exclude=("mu", "rho")):
    """Fraction of the band the built-for row of every query uses, the terms in `exclude` left out of the band."""
    q = np.arange(adv.queries.shape[0])
    r = adv.tight
    band = sum(t[q, r] for name, t in m["terms"].items() if name not in exclude)
    return (m["lhs"][q, r] - m["est"][q, r]) / band
