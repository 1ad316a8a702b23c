"""The path bench.py times - rmhmc_chains_run at BASELINE config 3 (8192 chains, D = 64, M = 10000, the int8 metric at 6 slices with
the certificate, default options, chains made stationary by 300 untimed steps) - against the CPU oracle at that size.

Everything the timed step adds to one transition is in play here and nowhere else at this size: hipGraph replay, the k_iter_begin /
k_iter_end state machine across transition boundaries, k_crestore and the c-tile cache, the row split of the 16-chains-per-wavefront
passes sized from the chain count (4 row ranges at 8192 chains, 16 in the small tests), and the delta assembly k_assemble_i8_sel,
whose 4-slice branch only stationary chains reach.  rmhmc_kernel_time's "i8_delta_*" counters show which slice counts the delta
assemblies really ran.

The oracle replays a chain c in a context of its own built from that chain's slice of the checkpoint (n = block length,
chain_offset = c, theta0 = the checkpoint's w, rmhmc_chains_restore with the saved counters): Philox is keyed by (seed, chain,
iteration), so it draws exactly the GPU's random numbers.

Measured on an MI355X (worst relative error of theta per chain over every state read; delta assemblies by slice count):
  stationary window, int8 at 6 slices   2.0e-13    end of step S' = 4 / 5 / 6: 30 / 0 / 0, inner iterate S' = 4 / 5: 30 / 0
  cold start, int8 at 6 slices          1.8e-12    end of step 1 / 25 / 14, inner iterate 1 / 39
  stationary window, fp64 matrix cores  1.2e-15    (no delta assembly)
The whole file takes about 20 s with 16 host cores; the two oracle comparisons, GPU runs included, about 7 s of it."""
import concurrent.futures

import numpy as np
import pytest

from conftest import rel_err
from riemannhamiltonianmontecarlo_amd import _capi
from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg

pytestmark = pytest.mark.gpu

M, D, N = 10000, 64, 8192
L, EPS, K, SEED = 6, 0.5, 4, 2024                       # bench.py: reference defaults, seed 2024
FLAGS = _capi.int8_metric_flags(6) | _capi.FLAG_INT8_CERTIFY
BURN_IN = 300
WINDOW = (6, 6, 18)                                     # 30 global steps, state read after each chunk
# per-chain bounds on theta: ten times the measured worst case (the trajectory bound of the other files is 1e-8)
TOL_I8 = 2e-12
TOL_I8_COLD = 2e-11
TOL_FP64 = 2e-14
# the first and last 16 chains and both sides of the 128-chain tile edges 127 / 128 and 4095 / 4096
EDGES = lambda n: sorted(set(range(16)) | {126, 127, 128, 129, n // 2 - 2, n // 2 - 1, n // 2, n // 2 + 1} | set(range(n - 16, n)))


@pytest.fixture(scope="session")
def problem():
    return synthetic_logreg(M, D, 0)


def _context(lib, problem, flags, n=None, options=None):
    ctx = lib.context(M, D, n or N, flags=flags, options=options)
    ctx.set_data(*problem)
    return ctx


@pytest.fixture(scope="module")
def i8ctx(hip, problem):
    ctx = _context(hip, problem, FLAGS)
    bound, active = ctx.int8_certificate()
    assert active and 0 < bound <= _capi.INT8_CERTIFY_TOL       # the int8 kernels are in use, as in the bench
    yield ctx
    ctx.close()


@pytest.fixture(scope="session")
def checkpoint(hip, problem):
    """(w, iters, accepted) after the bench's 300 untimed burn-in steps: stationary chains."""
    with _context(hip, problem, FLAGS) as ctx:
        ctx.chains_init(seed=SEED, L=L, eps=EPS, K=K)
        ctx.chains_run(BURN_IN)
        w, it, acc = ctx.chains_state()
    assert (it > 50).all() and (acc > 0).all() and np.isfinite(w).all()
    return w, it, acc


def _run_window(ctx, ck, chunks):
    """From checkpoint ck (None: theta0 = 1e-3, no counters), run the chunks of global steps; the state after each one."""
    if ck is None:
        ctx.chains_init(seed=SEED, L=L, eps=EPS, K=K)
    else:
        ctx.chains_init(theta0=ck[0], seed=SEED, L=L, eps=EPS, K=K)
        ctx.chains_restore(ck[1], ck[2])
    out = []
    for s in chunks:
        ctx.chains_run(s)
        out.append(ctx.chains_state())
    return out


def _blocks(chains):
    """sorted chain indices -> contiguous (start, stop) ranges"""
    out = []
    for c in sorted(set(int(c) for c in chains)):
        if out and out[-1][1] == c:
            out[-1][1] = c + 1
        else:
            out.append([c, c + 1])
    return [tuple(b) for b in out]


def _oracle_window(oracle, problem, ck, chains, chunks):
    """The oracle's states after each chunk for the given chains: one context per contiguous block (chain_offset = its first chain),
    the blocks side by side on host threads (the oracle's own OpenMP loop runs over the chains of one block)."""
    def one(block):
        a, b = block
        with _context(oracle, problem, 0, n=b - a) as ctx:
            if ck is None:
                ctx.chains_init(seed=SEED, chain_offset=a, L=L, eps=EPS, K=K)
            else:
                ctx.chains_init(theta0=ck[0][a:b], seed=SEED, chain_offset=a, L=L, eps=EPS, K=K)
                ctx.chains_restore(ck[1][a:b], ck[2][a:b])
            states = []
            for s in chunks:
                ctx.chains_run(s)
                states.append(ctx.chains_state())
            return states
    blocks = _blocks(chains)
    with concurrent.futures.ThreadPoolExecutor(max_workers=len(blocks)) as ex:
        res = list(ex.map(one, blocks))
    out = {}
    for (a, b), states in zip(blocks, res):
        for c in range(a, b):
            out[c] = [(w[c - a], it[c - a], acc[c - a]) for w, it, acc in states]
    return out


def _rejecters(states, ck, exclude, k=8):
    """k chains (spread over the batch) that rejected a proposal inside the window, outside `exclude`"""
    w, it, acc = states[-1]
    it0, acc0 = (ck[1], ck[2]) if ck is not None else (0, 0)
    rej = (it - it0) - (acc - acc0) > 0
    rej[list(exclude)] = False
    cand = np.nonzero(rej)[0]
    assert len(cand) >= k
    return [int(c) for c in cand[np.linspace(0, len(cand) - 1, k).astype(int)]]


def _compare(gpu_states, orc, ck, tol):
    """iters / accepted equal and theta within tol per chain at every state read; returns (worst error, rejections seen)"""
    worst, rejected = 0.0, 0
    for c, ostates in orc.items():
        for j, ((w, it, acc), (wo, ito, acco)) in enumerate(zip(gpu_states, ostates)):
            assert it[c] == ito and acc[c] == acco, (c, j, it[c], ito, acc[c], acco)
            e = rel_err(w[c], wo)
            worst = max(worst, e)
            assert e < tol, (c, j, e)
        it0, acc0 = (ck[1][c], ck[2][c]) if ck is not None else (0, 0)
        rejected += int((ostates[-1][1] - it0) - (ostates[-1][2] - acc0) > 0)
    return worst, rejected


_oracle_cache = {}


def _oracle_stationary(oracle, problem, ck, chains):
    key = tuple(sorted(chains))
    if key not in _oracle_cache:
        _oracle_cache[key] = _oracle_window(oracle, problem, ck, key, WINDOW)
    return _oracle_cache[key]


def test_stationary_window_matches_oracle(i8ctx, oracle, problem, checkpoint):
    """30 global steps (chunks of 6, 6, 18) from the stationary checkpoint: after the restore every chain starts a transition in
    lockstep, trajectories of 1 to 6 steps mix the phases and cross several transition boundaries.  48 chains against the oracle: the
    first and last 16, both sides of the tile edges 127 / 128 and 4095 / 4096, and 8 chains that rejected a proposal inside the window
    (k_crestore and the cdyn path); worst error 2.0e-13.  Every delta assembly of the window ran on 4 slices, at the end of a step
    (30 / 0 / 0 with S' = 4 / 5 / 6) and for the inner iterate (30 / 0) alike.
    The whole batch is held to the bits of the same window with cdyn = 0, where every momentum pass recomputes c itself (no c tile
    re-use, no k_crestore): a few hundred chains reject per step, and which of them a kernel mishandles is not for a sample to
    guess."""
    states = _run_window(i8ctx, checkpoint, WINDOW)
    counts = i8ctx.i8_delta_counts()
    i8ctx.set_option("cdyn", 0)
    try:
        plain = _run_window(i8ctx, checkpoint, WINDOW)
    finally:
        i8ctx.set_option("cdyn", 1)
    for j, (a, b) in enumerate(zip(states, plain)):
        for x, y in zip(a, b):
            assert np.array_equal(x, y), j
    chains = EDGES(N) + _rejecters(states, checkpoint, EDGES(N))
    orc = _oracle_stationary(oracle, problem, checkpoint, chains)
    worst, rejected = _compare(states, orc, checkpoint, TOL_I8)
    print("stationary int8: %d chains, worst theta error %.2e, %d rejected in the window; delta counts %s" % (len(orc), worst, rejected, counts))
    assert rejected >= 8
    assert counts["end"] == [sum(WINDOW), 0, 0], counts
    assert counts["inner"] == [sum(WINDOW), 0], counts


def test_cold_start_matches_oracle(i8ctx, oracle, problem):
    """40 global steps from theta0 = 1e-3 (no burn-in): the chains whose v exponent changes (re-based delta assemblies) and the
    wide differences that need 5 or 6 slices.  16 chains against the oracle: worst error 1.8e-12.  Delta assemblies at the end of a
    step with S' = 4 / 5 / 6: 1 / 25 / 14; inner iterate with S' = 4 / 5: 1 / 39 - one of each per global step."""
    chunks = (10, 10, 20)
    states = _run_window(i8ctx, None, chunks)
    counts = i8ctx.i8_delta_counts()
    chains = list(range(8)) + list(range(N - 8, N))
    orc = _oracle_window(oracle, problem, None, chains, chunks)
    worst, rejected = _compare(states, orc, None, TOL_I8_COLD)
    print("cold start int8: %d chains, worst theta error %.2e; delta counts %s" % (len(orc), worst, counts))
    assert sum(counts["end"]) == sum(chunks) and sum(counts["inner"]) == sum(chunks), counts
    assert counts["end"][1] + counts["end"][2] > 0 and counts["inner"][1] > 0, counts


def test_fp64_matrix_core_window_matches_oracle(hip, oracle, problem, checkpoint):
    """The same window on the fp64 matrix cores (flags = 0: bench.py's roofline_fp64 alternate), from the same checkpoint (its
    positions came from the int8 run; only the window is compared): worst error 1.2e-15.  No int8 delta assembly runs."""
    with _context(hip, problem, 0) as ctx:
        states = _run_window(ctx, checkpoint, WINDOW)
        counts = ctx.i8_delta_counts()
    chains = EDGES(N) + _rejecters(states, checkpoint, EDGES(N))
    orc = _oracle_stationary(oracle, problem, checkpoint, chains)
    worst, rejected = _compare(states, orc, checkpoint, TOL_FP64)
    print("stationary fp64: %d chains, worst theta error %.2e, %d rejected in the window" % (len(orc), worst, rejected))
    assert rejected >= 8
    assert counts == {"end": [0, 0, 0], "inner": [0, 0]}


def test_options_do_not_change_bits_at_bench_geometry(i8ctx, checkpoint):
    """graph = 0, inflight = 0, crestore = 0 and cdyn = 0 each give the bits of the default run, 30 steps from the checkpoint at the
    bench's own row split (the same comparisons elsewhere run 200 - 4096 chains with D <= 50)."""
    base = _run_window(i8ctx, checkpoint, (sum(WINDOW),))[-1]
    it, acc = base[1] - checkpoint[1], base[2] - checkpoint[2]
    assert (it > acc).sum() > N // 4                  # many chains rejected: k_crestore had work in the window
    for key in ("graph", "inflight", "crestore", "cdyn"):
        default = i8ctx.get_option(key)
        i8ctx.set_option(key, 0)
        try:
            other = _run_window(i8ctx, checkpoint, (sum(WINDOW),))[-1]
        finally:
            i8ctx.set_option(key, default)
        for a, b in zip(base, other):
            assert np.array_equal(a, b), key


# (flags, create-time options, bound on the relative difference of a resumed transition's theta: 0 = the same bits)
RESUME_VARIANTS = {"int8": (FLAGS, None, 1e-13), "int8_no_delta": (FLAGS, {"i8_delta": 0}, 0.0), "fp64": (0, None, 0.0)}


@pytest.mark.parametrize("variant", sorted(RESUME_VARIANTS))
def test_checkpoint_resume_at_bench_size(hip, problem, checkpoint, variant):
    """The 30-step window as 11 steps, a checkpoint, and the rest in a fresh context, against the window in one go: every transition
    both runs complete, on 64 chains spread over the batch (rmhmc_chains_restore, as bench.py --load-state and tools/profile.sh use it).
    fp64 matrix cores, and the int8 path with option i8_delta = 0: the same bits (0 of 496 transitions differ).  The int8 path with its
    default delta assembly: the uninterrupted run carried the metric at a chain's position forward as G(last position iterate) + the
    assembly of the difference, the resumed one assembles it in full from the position alone - the same integers, one fp64 rounding
    apart - so resumed transitions agree to the last bits only: 316 of 496 differ, by at most 3.8e-15 relative."""
    flags, options, tol = RESUME_VARIANTS[variant]
    sample = np.unique(np.linspace(0, N - 1, 64).astype(int))

    def visited(ctx, steps, seen, last):
        for _ in range(steps):
            ctx.chains_run(1)
            w, it, acc = ctx.chains_state()
            for c in sample:
                if it[c] > last[c]:
                    seen[c][int(it[c])] = w[c].copy(); last[c] = it[c]
        return ctx.chains_state()

    def start(ctx, ck):
        ctx.chains_init(theta0=ck[0], seed=SEED, L=L, eps=EPS, K=K)
        ctx.chains_restore(ck[1], ck[2])

    ref, got = {c: {} for c in sample}, {c: {} for c in sample}
    with _context(hip, problem, flags, options=options) as ctx:
        start(ctx, checkpoint)
        visited(ctx, sum(WINDOW), ref, checkpoint[1].copy())
        start(ctx, checkpoint)
        mid = visited(ctx, 11, got, checkpoint[1].copy())
    with _context(hip, problem, flags, options=options) as ctx:
        start(ctx, mid)
        visited(ctx, sum(WINDOW) - 11, got, mid[1].copy())
    n_common, n_diff, worst = 0, 0, 0.0
    for c in sample:
        common = sorted(set(ref[c]) & set(got[c]))
        assert len(common) >= 3 and common[-1] > mid[1][c], c       # transitions of both halves
        n_common += len(common)
        for k in common:
            e = rel_err(got[c][k], ref[c][k])
            n_diff += int(e > 0); worst = max(worst, e)
            assert e <= tol, (c, k, e)
    print("checkpoint / resume, %s: %d transitions compared on %d chains, %d differ, worst %.2e" % (variant, n_common, len(sample), n_diff, worst))
