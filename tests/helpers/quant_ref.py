"""NumPy restatement of include/rmhmc_quant.h, written from the header's prose: the key, the plan of the targets, the histogram partial of a
round, one step of the select, the finish, and the whole eight-round loop.  Independent of csrc/quant.h; tests compare the two bit for bit,
and both against np.sort."""
from fractions import Fraction

import numpy as np

SIGN = np.uint64(1 << 63)
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)
BINS, ROUNDS = 256, 8


def key(x):
    """order-preserving uint64 key of finite doubles: -0.0 made +0.0; all bits inverted where the sign is set, else the sign bit set"""
    x = np.ascontiguousarray(x, dtype=np.float64) + 0.0          # -0.0 + 0.0 = +0.0; everything else unchanged
    u = x.view(np.uint64)
    return np.where(u & SIGN != 0, u ^ ALL, u | SIGN)


def unkey(k):
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return np.where(k & SIGN != 0, k ^ SIGN, k ^ ALL).view(np.float64)


def digit(k, r):
    return ((k >> np.uint64(56 - 8 * r)) & np.uint64(255)).astype(np.int64)


def carry_mask(r):
    """the bits of a prefix under the digits of rounds 0 .. r"""
    return 0 if r >= 7 else (1 << (56 - 8 * r)) - 1


def plan(m, probs):
    m = np.asarray(m, dtype=np.int64)
    probs = np.atleast_1d(np.asarray(probs, dtype=np.float64))
    Q, P = probs.size, m.size
    rank = np.full((2 * Q, P), -1, dtype=np.int64)
    frac = np.zeros((Q, P))
    for j, q in enumerate(probs):
        for d in range(P):
            if m[d] > 0:
                h = float(m[d] - 1) * float(q)
                lo = int(np.floor(h))
                rank[2 * j, d], rank[2 * j + 1, d], frac[j, d] = lo, min(lo + 1, m[d] - 1), h - np.floor(h)
    return rank, frac


def hist(x, r, prefix=None):
    """the histogram partial of round r of x [..., P] (any leading shape): [1][P][256] in round 0, [K][P][256] afterwards"""
    x = np.asarray(x, dtype=np.float64)
    P = x.shape[-1]
    x = x.reshape(-1, P)
    Kh = 1 if r == 0 else len(prefix)
    out = np.zeros((Kh, P, BINS))
    for d in range(P):
        col = x[:, d]
        k = key(col[np.isfinite(col)])
        for t in range(Kh):
            kk = k
            if r > 0:
                sh = np.uint64(64 - 8 * r)
                kk = k[(k >> sh) == (np.uint64(prefix[t][d]) >> sh)]
            out[t, d] = np.bincount(digit(kk, r), minlength=BINS)
    return out


def step(hists, r, prefix, rank):
    """one round on the sum of `hists`, prefix (uint64 [K][P]) and rank (int64 [K][P]) updated in place; ValueError, nothing written,
    for a histogram that does not continue the previous round"""
    h = np.sum([np.asarray(p, dtype=np.float64) for p in hists], axis=0)
    K, P = prefix.shape
    newp, newr = prefix.copy(), rank.copy()
    for t in range(K):
        for d in range(P):
            if rank[t, d] < 0:
                continue
            c = [int(v) for v in h[t if r else 0, d]]
            total = sum(c)
            old = int(prefix[t, d])
            if total <= rank[t, d]:
                raise ValueError("total not above the rank")
            if r:
                cm = carry_mask(r - 1)
                want = old & cm
                if (total != want) if want < cm else (total < cm):
                    raise ValueError("total is not the count of the bin chosen before")
            cum, b = 0, 0
            while cum + c[b] <= rank[t, d]:
                cum += c[b]
                b += 1
            newr[t, d] = rank[t, d] - cum
            digits = (old & ~carry_mask(r - 1)) if r else 0
            newp[t, d] = np.uint64((digits & (2 ** 64 - 1)) | (b << (56 - 8 * r)) | min(c[b], carry_mask(r)))
    prefix[...] = newp
    rank[...] = newr


def finish_exact(lo, hi, g):
    """g == 0 ? lo : fma(g, hi - lo, lo) of scalars, the fma in exact rational arithmetic and rounded once"""
    lo, hi, g = float(lo), float(hi), float(g)
    return lo if g == 0.0 else float(Fraction(g) * Fraction(hi - lo) + Fraction(lo))


def finish(prefix, frac, m):
    Q, P = frac.shape
    out = np.full((Q, P), np.nan)
    x = unkey(prefix)
    for j in range(Q):
        for d in range(P):
            if m[d] > 0:
                out[j, d] = finish_exact(x[2 * j, d], x[2 * j + 1, d], frac[j, d])
    return out


def select(x, probs, splits=None):
    """the whole loop on x [..., P]; splits: row ranges of the flattened x that play the shards (default: one).  Returns dict(quantiles
    [Q][P], draws_used [P], order: the order statistics [2Q][P], rank0: their ranks)"""
    x = np.asarray(x, dtype=np.float64)
    P = x.shape[-1]
    x = x.reshape(-1, P)
    splits = splits or [(0, len(x))]
    h0 = [hist(x[a:b], 0) for a, b in splits]
    m = np.sum(h0, axis=0)[0].sum(axis=1).astype(np.int64)
    rank, frac = plan(m, probs)
    rank0 = rank.copy()
    prefix = np.zeros(rank.shape, dtype=np.uint64)
    step(h0, 0, prefix, rank)
    for r in range(1, ROUNDS):
        step([hist(x[a:b], r, prefix) for a, b in splits], r, prefix, rank)
    return dict(quantiles=finish(prefix, frac, m), draws_used=m, order=unkey(prefix), rank0=rank0, frac=frac)


def sorted_stats(x, probs):
    """what np.sort gives: per dimension the finite values sorted; (order statistics [2Q][P] at the plan's ranks with -0.0 read as +0.0 and
    NaN where there is none, quantiles [Q][P] by the exact finish, m [P])"""
    x = np.asarray(x, dtype=np.float64)
    P = x.shape[-1]
    x = x.reshape(-1, P)
    m = np.isfinite(x).sum(axis=0).astype(np.int64)
    rank, frac = plan(m, probs)
    order = np.full(rank.shape, np.nan)
    quant = np.full(frac.shape, np.nan)
    for d in range(P):
        col = np.sort(x[np.isfinite(x[:, d]), d]) + 0.0
        for t in range(rank.shape[0]):
            if rank[t, d] >= 0:
                order[t, d] = col[rank[t, d]]
        for j in range(frac.shape[0]):
            if m[d] > 0:
                quant[j, d] = finish_exact(order[2 * j, d], order[2 * j + 1, d], frac[j, d])
    return order, quant, m


def same_bits(a, b):
    """equal as bit patterns (so NaN equals NaN and +0.0 differs from -0.0)"""
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | nan).all())


def edge_data(seed, N, P):
    """[N][P] whose columns cycle through the cases that exercise the rounds: constant; values that differ only in the lowest byte; mixed
    signs with +-0; denormals; scattered NaN and +-inf; entirely NaN; ordinary normal draws"""
    rs = np.random.RandomState(seed)
    x = np.empty((N, P))
    for d in range(P):
        c = d % 7
        if c == 0:
            col = np.full(N, -3.75)
        elif c == 1:
            col = (np.float64(1.5).view(np.uint64) + rs.randint(0, 256, N).astype(np.uint64)).view(np.float64)
        elif c == 2:
            col = rs.randn(N)
            col[rs.rand(N) < 0.3] = 0.0
            col[rs.rand(N) < 0.2] = -0.0
        elif c == 3:
            col = rs.randint(-2000, 2000, N) * 5e-324
        elif c == 4:
            col = rs.randn(N) * 1e3
            col[rs.rand(N) < 0.1] = np.nan
            col[rs.rand(N) < 0.05] = np.inf
            col[rs.rand(N) < 0.05] = -np.inf
        elif c == 5:
            col = np.full(N, np.nan)
        else:
            col = 2.0 + 0.3 * rs.randn(N)
        x[:, d] = col
    return x
