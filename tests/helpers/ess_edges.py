"""Harness of tests/test_ess_edges_cpu.py and tests/test_gpu_ess_edges.py: the ESS / mean / variance kernel k_ess (csrc/kernels.hip.h)
and the run-mean kernel k_run_mean (csrc/output.hip.h) at their edges.

k_ess gives one wavefront a series: lane `lane` walks s = lane, lane + 64, ... for the mean, the centred copy in LDS and every lag
product, with and without a lag offset; the block index is (chain, dimension) = (idx / P, idx % P) and the loads have stride P.  With
RMHMC_FLAG_ESS_WRAP lag l also receives the linear lag nfft - l, nfft = nextpow2(S) + 1 (tools.py:16-23): that term exists only for
l >= nfft - S + 1, so only a series whose length is at or just below a power of two can show it before the Geyer sum stops.

ess_ld: the estimator of tools.py:21-74 lag by lag in np.longdouble, no FFT - the reference of both test files.
kernel_restatement: the same estimator in float64 the way the kernel sums (64 strided partial sums and a butterfly), CPU only, with
named mutations: tests/test_ess_edges_cpu.py shows that the case table below tells every mutated kernel from a right one.
CASES: the table.  GPU-free; every input and reference is computed once per process, shared and read-only.

Three mutations need a word, because the form the kernel is written in makes their literal reading no error at all:
  wrap_at_lag0       nfft - 0 = nfft > S: a wrapped partner of lag 0 taken literally is an empty sum.  The error that exists is the
                     circular one, partner (nfft - l) mod nfft = 0: lag 0 counted twice in Gamma_0.  That is what the mutation does.
  stop_on_raw_pair   min(Gamma_0..Gamma_j) <= 0 first happens at the first raw Gamma_j <= 0, so a loop that tests the raw pair before
                     the clamp stops where the kernel stops.  The error that exists is the one of the reference's own form
                     (tools.py:62-67 counts the positive entries, then sums that many): the count taken over the raw pairs.
  half_rounds_up     half = (S + 1) / 2 adds, for odd S, the pair (S - 1, S) to a sum that has run through every pair.  For a centred
                     series the autocorrelations of all lags >= 1 sum to -1/2, so that sum is 1/2 - rho_(S-1) and, with the extra pair
                     (at most rho_(S-1) after the clamp), at most 1/2: tau = -1 + 2 sum <= 0 is raised to 1 and the ESS is S either
                     way.  In wrap mode the same held for each of over 30 000 never-stopping columns of S = 3 ... 63 that were searched.
                     No input can show it: it is listed in EQUIVALENT, and the CPU test asserts that it changes nothing in a table
                     that does hold odd-length series which never stop, instead of asserting that a case catches it."""
import collections

import numpy as np

from riemannhamiltonianmontecarlo_amd import tools

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "np.longdouble is no wider than float64 here: ess_ld would be no reference"

S_MAX = 20000                 # launch_ess: S doubles of LDS per wavefront
MARGIN = 1e-6                 # out_ref.ess_ref: a Geyer pair sum this close to 0 makes an ESS comparison meaningless
ESS_RTOL = 1e-9               # tests/test_gpu_out.py
MEAN_TOL = dict(rtol=1e-12, atol=1e-14)

_cache = {}


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def nfft_of(S, mode):
    """what launch_ess passes: 0 in linear mode, nextpow2(S) + 1 with RMHMC_FLAG_ESS_WRAP"""
    return tools.nextpow2(S) + 1 if mode == "wrap" else 0


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------
def ess_ld(x, nfft=0):
    """x (S, P) float64.  Per column, in np.longdouble: mean, centred series, c0, Gamma_j = (a_2j + a_2j+1) / c0 with a_l the linear
    autocovariance sum (plus the one of lag nfft - l when nfft > 0 and l > 0), running minimum, sum while > 0, tau = max(1, -1 + 2 sum),
    ess = S / tau.  Returns dict(ess, mean, var (population), pairs: the number of pairs summed, margin: the smallest |Gamma_j| of the
    running minimum up to and including the stopping pair (out_ref.geyer_margin), clamped: the summed pairs the running minimum
    changed), float64 [P] and int64 [P].  A column with a NaN or an inf has ess, mean and var NaN; a constant column has its mean,
    var 0 and ess NaN (include/rmhmc_out.h); their margin is inf, as they take part in no ESS comparison."""
    x = np.asarray(x, dtype=np.float64)
    S, P = x.shape
    finite = np.isfinite(x).all(axis=0)
    X = np.where(finite[None, :], x, 0.0).astype(LD)
    m = X.sum(axis=0) / LD(S)
    v = X - m
    c0 = (v * v).sum(axis=0)
    half = S // 2
    active = finite & (c0 > 0)
    total = np.zeros(P, dtype=LD); prev = np.full(P, np.inf, dtype=LD); margin = np.full(P, np.inf)
    pairs = np.zeros(P, dtype=np.int64); clamped = np.zeros(P, dtype=np.int64)

    def lag(vv, l):
        return (vv[:S - l] * vv[l:]).sum(axis=0) if 0 <= l < S else LD(0)

    for j in range(half):
        cols = np.flatnonzero(active)
        if cols.size == 0:
            break
        vv = v[:, cols]
        a = lag(vv, 2 * j) + lag(vv, 2 * j + 1)
        if nfft > 0:
            if j > 0:
                a = a + lag(vv, nfft - 2 * j)
            a = a + lag(vv, nfft - 2 * j - 1)
        raw = a / c0[cols]
        g = np.minimum(raw, prev[cols])
        margin[cols] = np.minimum(margin[cols], np.abs(g).astype(np.float64))
        pos = g > 0
        on = cols[pos]
        total[on] += g[pos]; prev[on] = g[pos]; pairs[on] += 1
        clamped[on] += (raw > g)[pos]
        active[cols[~pos]] = False
    tau = np.maximum(LD(1), LD(-1) + LD(2) * total)
    ok = finite & (c0 > 0)
    return dict(ess=np.where(ok, (LD(S) / tau), np.nan).astype(np.float64), mean=np.where(finite, m, np.nan).astype(np.float64),
                var=np.where(finite, c0 / LD(S), np.nan).astype(np.float64), pairs=pairs, margin=margin, clamped=clamped)


def columns(x):
    """[n][S][P] -> (S, n P): the series of block index c P + d in column c P + d"""
    x = np.asarray(x)
    n, S, P = x.shape
    return np.ascontiguousarray(x.transpose(1, 0, 2).reshape(S, n * P))


def block_ref(x, nfft):
    """ess_ld of a block [n][S][P]: every array [n][P]"""
    n, S, P = np.asarray(x).shape
    return {k: a.reshape(n, P) for k, a in ess_ld(columns(x), nfft).items()}


# ---- the kernel, restated, with its mutations ------------------------------------------------------------------------------------------------
MUTATIONS = ("no_wrap", "wrap_off_by_one_low", "wrap_off_by_one_high", "wrap_at_lag0", "drop_last_row", "drop_row_63", "half_rounds_up",
             "no_monotone_clamp", "stop_on_raw_pair", "var_sample", "no_c0_guard", "mean_of_inf_column")
EQUIVALENT = ("half_rounds_up",)    # no input tells it from the kernel: see the module's docstring
ALL_PAIRS_S_MAX = 2000        # stop_on_raw_pair evaluates every pair: S^2 / 2 products per column, kept to the cases where that is cheap


def _wave_sum(terms, drop_row_63=False):
    """terms (m, P) in the order of s: lane l adds its terms l, l + 64, ... in that order, then the butterfly of wave_sum"""
    m, P = terms.shape
    if drop_row_63 and m > 63:
        terms = terms.copy(); terms[63] = 0.0
    rows = -(-m // 64)
    t = np.zeros((rows * 64, P)); t[:m] = terms
    t = t.reshape(rows, 64, P)
    lanes = np.zeros((64, P))
    for r in range(rows):
        lanes = lanes + t[r]
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[idx ^ o]
    return lanes[0]


def kernel_restatement(x, nfft=0, mutation=None):
    """x (S, P) float64 -> dict(ess, mean, var) float64 [P], as k_ess computes them (fma not reproduced)"""
    assert mutation is None or mutation in MUTATIONS, mutation
    x = np.asarray(x, dtype=np.float64)
    S, P = x.shape
    end = S - 1 if mutation == "drop_last_row" else S
    d63 = mutation == "drop_row_63"
    if mutation == "no_wrap":
        nfft = 0
    shift = {"wrap_off_by_one_low": -1, "wrap_off_by_one_high": 1}.get(mutation, 0)
    with np.errstate(all="ignore"):
        m = _wave_sum(x[:end], d63) / S
        v = x - m
        c0 = _wave_sum(v[:end] * v[:end], d63)

        def lag(vv, l):
            return _wave_sum(vv[:end - l] * vv[l:end], d63) if 0 <= l < end else np.zeros(vv.shape[1])

        half = (S + 1) // 2 if mutation == "half_rounds_up" else S // 2
        all_pairs = mutation == "stop_on_raw_pair"
        assert not all_pairs or S <= ALL_PAIRS_S_MAX
        active = np.ones(P, dtype=bool)
        total = np.zeros(P); prev = np.full(P, np.inf); npos_raw = np.zeros(P, dtype=np.int64)
        gammas = []
        for j in range(half):
            cols = np.flatnonzero(active)
            if cols.size == 0:
                break
            vv = v[:, cols]
            l0, l1 = 2 * j, 2 * j + 1
            a = lag(vv, l0); b = lag(vv, l1)
            if nfft > 0:
                if l0 > 0:
                    a = a + lag(vv, nfft - l0 + shift)
                elif mutation == "wrap_at_lag0":
                    a = a + lag(vv, 0)                    # (nfft - 0) mod nfft
                b = b + lag(vv, nfft - l1 + shift)
            g = (a + b) / c0[cols]
            if all_pairs:                                 # every column stays active: the count is taken over all raw pairs
                npos_raw += g > 0
                g = np.minimum(g, prev); prev = g
                gammas.append(g)
                continue
            if mutation != "no_monotone_clamp":
                g = np.where(g > prev[cols], prev[cols], g)
            pos = g > 0
            on = cols[pos]
            total[on] += g[pos]; prev[on] = g[pos]
            active[cols[~pos]] = False
        if all_pairs:
            csum = np.vstack([np.zeros((1, P)), np.cumsum(np.array(gammas).reshape(-1, P), axis=0)])
            total = csum[npos_raw, np.arange(P)]
        mono = np.maximum(1.0, -1.0 + 2.0 * total)
        mono = np.where(mono < 1.0, 1.0, mono)            # (a NaN sum cannot arise: a NaN pair stops the loop before it is added)
        ess = S / mono if mutation == "no_c0_guard" else np.where(c0 > 0, S / mono, np.nan)
        mean = m if mutation == "mean_of_inf_column" else np.where(c0 == c0, m, np.nan)
        var = c0 / (S - 1 if mutation == "var_sample" else S)
    return dict(ess=ess, mean=mean, var=var)


def block_restatement(x, nfft, mutation=None):
    n, S, P = np.asarray(x).shape
    return {k: a.reshape(n, P) for k, a in kernel_restatement(columns(x), nfft, mutation).items()}


# ---- comparisons -----------------------------------------------------------------------------------------------------------------------------
def errors(got, ref):
    """dict(ess: the largest relative error where the reference has an ESS and its Geyer margin is above MARGIN, mean / var: the largest
    excess over MEAN_TOL in units of that tolerance (<= 1 passes), nan: whether the NaN patterns of all three agree)"""
    out = dict(nan=all(np.array_equal(np.isnan(got[k]), np.isnan(ref[k])) for k in ("ess", "mean", "var")))
    with np.errstate(all="ignore"):
        use = np.isfinite(ref["ess"]) & (ref["margin"] > MARGIN)
        e = np.abs(np.asarray(got["ess"])[use] / ref["ess"][use] - 1.0)
        out["ess"] = float(np.nan_to_num(e, nan=np.inf).max()) if e.size else 0.0
        for k in ("mean", "var"):
            fin = np.isfinite(ref[k])
            r = np.abs(np.asarray(got[k])[fin] - ref[k][fin]) / (MEAN_TOL["atol"] + MEAN_TOL["rtol"] * np.abs(ref[k][fin]))
            out[k] = float(np.nan_to_num(r, nan=np.inf).max()) if r.size else 0.0
    return out


def rel_diff(got, ref, k):
    """the largest relative difference of quantity k over the entries where both are finite"""
    with np.errstate(all="ignore"):
        a, b = np.asarray(got[k], dtype=np.float64), np.asarray(ref[k], dtype=np.float64)
        fin = np.isfinite(a) & np.isfinite(b) & (b != 0)
        if k == "ess":
            fin &= ref["margin"] > MARGIN
        return float(np.abs(a[fin] / b[fin] - 1.0).max()) if fin.any() else 0.0


# ---- the case table ------------------------------------------------------------------------------------------------------------------------
# gen: ("ar", phis, seed) AR(1) of unit innovations from its stationary law, column d with phi = phis[d % len(phis)];
#      ("alt", seed) x_s = (-1)^s (1 + 1e-3 z_s);  ("ar_outlier", phi, seed) AR(1) with row S - 1 moved up by 30 standard deviations;
#      ("nonfinite", kind, seed) the AR block of that seed with the entry, column or chain of `kind` planted (plant below).
# offset: added per column in units of that column's standard deviation; scale: a power of two, applied last (exact).
Case = collections.namedtuple("Case", "id n S P gen offset scale mode why")
PHIS = (0.0, 0.5, 0.9)
WRAP_PHIS = (0.5, 0.9)        # the wrapped lags carry weight only in a series that is still correlated at lag nfft - S + 1


def _c(id, n, S, P, gen, mode="linear", offset=0.0, scale=1.0, why=""):
    return Case(id, n, S, P, gen, offset, scale, mode, why)


SIZES_LINEAR = (2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 1000)
SIZES_WRAP = (8, 16, 64, 128, 37, 65)
WRAP_REACHED = (8, 16, 64, 128)          # S a power of two: nfft - S + 1 = 2, every lag from 2 on has a wrapped partner
WRAP_NOT_REACHED = (37, 65)              # the first wrapped lag is 29 / 65: beyond where these sums stop (S = 65: beyond the series)
ALT_S = (2, 3, 64, 129)
WIDTHS = (1, 3, 65, 130)
OFFSETS = (0.0, 1e4, 1e8)
SCALES = (-300, -40, 0, 40, 300)
NONFINITE = ("const", "nan", "pinf", "ninf", "nan_tail")
FIRST_PAIR_SEED, CLAMP_SEED = 9, 78   # the first seeds with the property; tests/test_ess_edges_cpu.py asserts it of each

CASES = []
for _S in SIZES_LINEAR:
    CASES.append(_c("size-lin-s%d" % _S, 3, _S, 5, ("ar", PHIS, 100 + _S),
                    why="half = %d, %d stride(s) of 64, last stride holds %d" % (_S // 2, -(-_S // 64), _S - 64 * ((_S - 1) // 64))))
CASES.append(_c("size-lin-s20000", 2, S_MAX, 2, ("ar_outlier", 0.5, 7),
                why="the limit: 160 000 B of LDS; row S - 1 holds an outlier of 30 sd; stops after a few pairs"))
for _S in SIZES_WRAP:
    # (S = 8, 16: most short series have tau clamped to 1 in both modes; these phis and seeds leave the wrap visible in over half of them)
    _gen = {8: ("ar", (0.9, 0.99), 204), 16: ("ar", (0.9, 0.99), 221)}.get(_S, ("ar", WRAP_PHIS, 200 + _S))
    CASES.append(_c("size-wrap-s%d" % _S, 3, _S, 5, _gen, mode="wrap",
                    why="nfft = %d: lags >= %d wrap" % (nfft_of(_S, "wrap"), nfft_of(_S, "wrap") - _S + 1)))
CASES.append(_c("size-wrap-s20000", 2, S_MAX, 2, ("ar_outlier", 0.5, 7), mode="wrap", why="nfft = 32769: no wrapped lag is reached"))
for _P in WIDTHS:
    for _mode in ("linear", "wrap"):
        CASES.append(_c("width-%s-p%d" % (_mode[:3], _P), 7, 64, _P, ("ar", WRAP_PHIS, 300 + _P), mode=_mode,
                        why="%d series: no multiple of 64 or 256; stride-%d loads" % (7 * _P, _P)))
for _S in ALT_S:
    for _mode in ("linear", "wrap"):
        CASES.append(_c("alt-%s-s%d" % (_mode[:3], _S), 2, _S, 3, ("alt", 400 + _S), mode=_mode,
                        why="every Gamma_j about 1 / S > 0: the sum runs through all %d pairs" % (_S // 2)))
CASES.append(_c("stop-first-pair", 1, 100, 3, ("ar", (0.0,), FIRST_PAIR_SEED), why="white noise with Gamma_1 <= 0 in every column"))
CASES.append(_c("clamp-fires", 1, 200, 3, ("ar", (0.9,), CLAMP_SEED), why="a summed pair is cut down to the running minimum"))
for _o in OFFSETS:
    CASES.append(_c("offset-%g" % _o, 4, 1000, 5, ("ar", (0.7,), 500), offset=_o, why="column means of %g standard deviations" % _o))
for _k in SCALES:
    if _k != 0:
        CASES.append(_c("scale-2^%d" % _k, 4, 1000, 5, ("ar", (0.7,), 500), scale=2.0 ** _k,
                        why="offset-0 times 2^%d: c0 about 2^%d, normal in float64" % (_k, 2 * _k + 10)))
for _kind in NONFINITE:
    CASES.append(_c("nonfinite-%s" % _kind, 3, 65, 4, ("nonfinite", _kind, 600), why="chain 1, column 2 (nan_tail: chain 1 from row 40 on)"))
    CASES.append(_c("nonfinite-%s-wrap" % _kind, 3, 64, 4, ("nonfinite", _kind, 601), mode="wrap", why="the same in wrap mode at S = 64"))
CASE = {c.id: c for c in CASES}
assert len(CASE) == len(CASES)
SCALE_BASE = "offset-0"
PLANT_AT = (1, 2)             # (chain, column) of the planted series
CONST_VALUE = 2.5             # S x 2.5 and every partial sum of it are exact in float64: the mean is exact, the centred series 0


def _ar(rs, n, S, P, phis):
    phi = np.array([phis[d % len(phis)] for d in range(P)])
    x = np.empty((n, S, P))
    x[:, 0] = rs.randn(n, P) / np.sqrt(1.0 - phi * phi)
    e = rs.randn(n, S, P)
    for s in range(1, S):
        x[:, s] = phi * x[:, s - 1] + e[:, s]
    return x


def plant(x, kind):
    """a copy of the block with the non-finite series of `kind` at PLANT_AT"""
    x = x.copy()
    c, d = PLANT_AT
    if kind == "const":
        x[c, :, d] = CONST_VALUE
    elif kind == "nan":
        x[c, 17, d] = np.nan
    elif kind == "pinf":
        x[c, x.shape[1] - 1, d] = np.inf
    elif kind == "ninf":
        x[c, 0, d] = -np.inf
    elif kind == "nan_tail":
        x[c, 40:, :] = np.nan
    else:
        raise ValueError(kind)
    return x


def base_block(case):
    """the block before offset, scale and planting (for a non-finite case: its finite twin)"""
    key = ("base", case.n, case.S, case.P, case.gen)
    if key not in _cache:
        kind, seed = case.gen[0], case.gen[-1]
        rs = np.random.RandomState(seed)
        if kind == "alt":
            sign = np.where(np.arange(case.S) % 2 == 0, 1.0, -1.0)[None, :, None]
            x = sign * (1.0 + 1e-3 * rs.randn(case.n, case.S, case.P))
        elif kind == "ar":
            x = _ar(rs, case.n, case.S, case.P, case.gen[1])
        elif kind == "ar_outlier":
            x = _ar(rs, case.n, case.S, case.P, (case.gen[1],))
            x[:, case.S - 1] += 30.0 / np.sqrt(1.0 - case.gen[1] ** 2)
        elif kind == "nonfinite":
            x = _ar(rs, case.n, case.S, case.P, WRAP_PHIS)
        else:
            raise ValueError(kind)
        x.setflags(write=False)
        _cache[key] = x
    return _cache[key]


def case_block(case):
    """the input of the case: float64 [n][S][P], read-only"""
    key = ("block", case.id)
    if key not in _cache:
        x = base_block(case)
        if case.offset:
            x = x + case.offset * x.std(axis=1, keepdims=True)
        if case.scale != 1.0:
            x = x * case.scale
        if case.gen[0] == "nonfinite":
            x = plant(x, case.gen[1])
        x = np.ascontiguousarray(x)
        x.setflags(write=False)
        _cache[key] = x
    return _cache[key]


def case_ref(case, mode=None):
    """ess_ld of the case's block in `mode` (default: the case's own): arrays [n][P]"""
    mode = mode or case.mode
    key = ("ref", case.id, mode)
    if key not in _cache:
        _cache[key] = _freeze(block_ref(case_block(case), nfft_of(case.S, mode)))
    return _cache[key]


def host_restatement(x, mode):
    """the float64 host restatement the offset bound is measured on: tools.CalculateESS and the two-pass NumPy mean and variance"""
    x = np.asarray(x)
    n, S, P = x.shape
    nf = "python" if mode == "wrap" else "matlab"
    return dict(ess=np.stack([tools.CalculateESS(x[c], S - 1, nf).ravel() for c in range(n)]), mean=x.mean(axis=1), var=x.var(axis=1))


HARD_OFFSET = "offset-1e+08"
assert HARD_OFFSET in CASE


def case_bounds(case, mode=None):
    """dict(ess: rtol, mean, var: in units of MEAN_TOL) a kernel is held to.  The project's tolerances, except at a mean of 1e8 standard
    deviations, where float64 itself is off: ten times the error of the float64 host restatement measured on the same inputs (the
    kernel's mean is 64 strided partial sums and a tree: the same order of error with another constant), and never below the project's
    tolerance - a host error that happens to be 0 asks no more of a kernel than every other case does.  With host: the measured errors."""
    mode = mode or case.mode
    if case.id != HARD_OFFSET:
        return dict(ess=ESS_RTOL, mean=1.0, var=1.0)
    key = ("bounds", mode)
    if key not in _cache:
        h = errors(host_restatement(case_block(case), mode), case_ref(case, mode))
        _cache[key] = dict(ess=max(10 * h["ess"], ESS_RTOL), mean=max(10 * h["mean"], 1.0), var=max(10 * h["var"], 1.0), host=h)
    return _cache[key]


# ---- placement -------------------------------------------------------------------------------------------------------------------------------
PLACE_S = 129
PLACE_BLOCKS = ((1, 1), (7, 3), (3, 65), (2, 130))


def placements(n, P):
    """the first, a middle and the last (chain, column) of a block"""
    return sorted({(0, 0), (n // 2, P // 2), (n - 1, P - 1)})


def place_series():
    if "place" not in _cache:
        x = _ar(np.random.RandomState(700), 1, PLACE_S, 1, (0.9,))[0, :, 0]
        x.setflags(write=False)
        _cache["place"] = x
    return _cache["place"]


def place_block(n, P, c, d):
    """a block of other series (AR(1) about a mean of 3, so that a wrong stride or index shows) with the series at (c, d)"""
    x = 3.0 + _ar(np.random.RandomState(701 + 1000 * n + P), n, PLACE_S, P, PHIS)
    x[c, :, d] = place_series()
    return x


# ---- the run-mean kernel ---------------------------------------------------------------------------------------------------------------------
# (n, S, D): S D = 255, 255, 256, 257, 259 on both sides of the 256-thread block; n on both sides of the chain loop's unroll of 8
RUN_MEAN_SHAPES = ((1, 51, 5), (7, 51, 5), (8, 64, 4), (9, 257, 1), (17, 37, 7))
RUN_MEAN_M = 200


def run_mean_def(x):
    """the chains added in order, one division"""
    acc = np.zeros(x.shape[1:])
    for c in range(x.shape[0]):
        acc = acc + x[c]
    return acc / x.shape[0]
