"""Posterior quantiles of include/rmhmc_quant.h on the GPU: the histogram partial of k_quant_hist / k_quant_out round by round against
the NumPy restatement tests/helpers/quant_ref.py, and the finished quantiles against np.sort of the host copy, at the smallest shapes at
which each edge of the kernel can go wrong; rmhmc_quant_dev against the composition of its pieces; determinism; chain splits; the
refusals; sample_to(quantiles=...); and multi_gpu.sample_sharded(quantiles=...) under three gloo ranks on the one GPU.

No tolerance anywhere: counts are integers, order statistics are np.sort's values, and an interpolated value is the exact rational
g (hi - lo) + lo rounded once (quant_ref.finish_exact).  The kernel walks the targets one at a time, so every target is a group
boundary; K = 1 and K = 16 bound the walk.  Needs an MI355X: run with pytest -m gpu."""
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from conftest import ROOT, synthetic_logreg
from riemannhamiltonianmontecarlo_amd import _capi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import diag_ref  # noqa: E402
import quant_ref as R  # noqa: E402
import sharded_quant_child as child  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PROBS = (0.025, 0.25, 0.5, 0.75, 0.975)
TILE = _capi.QUANT_MAX_TILE                      # widest column tile
ROWS_WIDE = _capi.quant_tile(TILE)[1]            # rows of a row block at that tile
ROWS_ONE = _capi.quant_tile(1)[1]                # ... and at one column
ROWS_16 = _capi.quant_tile(15)[1]
# (seed, n, S, P): N = n S rows
SHAPES = {
    "one_value": (1, 1, 1, 1),                                   # n S = 1, P = 1
    "one_column_block_minus_1": (2, 1, ROWS_ONE - 1, 1),         # P = 1: every lane of a wavefront holds the same column
    "one_column_block_plus_1": (3, 1, ROWS_ONE + 1, 1),          # ... and a second row block of one row
    "tile_minus_1": (4, 3, (ROWS_WIDE + 1) // 3 + 1, TILE - 1),  # one column fewer than a tile, more than one row block
    "tile_plus_1": (5, 1, ROWS_WIDE - 1, TILE + 1),              # P = 65: a second tile of one column; one row fewer than a row block
    "two_tiles_block_plus_1": (6, 1, ROWS_WIDE + 1, 2 * TILE + 3),
    "narrow_tile": (7, 2, ROWS_16 // 2 + 3, 15),                 # the australian width: 4 lanes of a wavefront share a column
    "narrow_tile_ragged": (8, 1, 2 * ROWS_16 + 1, 17),           # 17 of 32 columns
    "two_columns": (9, 5, 1000, 2),
    "three_columns": (11, 2, 500, 3),                            # a tile of 4
    "seven_columns": (12, 2, 500, 7),                            # a tile of 8
    "ar1": (10, 40, 300, 33),                                    # an AR(1) posterior-like tensor, 396 000 values
}
_inputs = {}


def inputs(name):
    """the tensor of a shape [n][S][P] and what np.sort says about it, computed once"""
    if name not in _inputs:
        seed, n, S, P = SHAPES[name]
        x = diag_ref.ar1(seed, n, S, P) if name == "ar1" else R.edge_data(seed, n * S, P).reshape(n, S, P)
        if name == "one_value":
            x[...] = -0.0
        elif P == 1:                      # (edge_data's first column is the constant one: take the one with NaN and infinities)
            x = np.ascontiguousarray(R.edge_data(seed, n * S, 5)[:, 4:5]).reshape(n, S, 1)
        _inputs[name] = (x, R.sorted_stats(x, PROBS))
    return _inputs[name]


@pytest.fixture(scope="module")
def ctx(hip):
    with hip.context(20, 2, 1) as c:      # the quantiles read samples of any shape: the context only names the GPU and the stream
        yield c


@pytest.mark.parametrize("name", list(SHAPES))
def test_quantiles_are_np_sort(ctx, name):
    x, (order, quant, m) = inputs(name)
    got = ctx.quantiles(torch.from_numpy(x).to(DEV), PROBS)
    assert isinstance(got["quantiles"], np.ndarray) and got["quantiles"].shape == (len(PROBS), x.shape[2])
    assert np.array_equal(got["draws_used"], m)
    assert R.same_bits(got["quantiles"], quant)
    if name == "one_value":
        assert (got["quantiles"] == 0.0).all() and not np.signbit(got["quantiles"]).any()      # a returned zero is +0.0


@pytest.mark.parametrize("name", ["tile_plus_1", "narrow_tile", "one_column_block_plus_1"])
def test_every_round_against_the_restatement(ctx, name):
    """K = 10; every round's partial equals the plain count, and the call equals the composition of its pieces"""
    x, (order, quant, m) = inputs(name)
    t = torch.from_numpy(x).to(DEV)
    P = x.shape[2]
    seen = []

    def hist(r, prefix, K):
        h = ctx.quant_hist(t, r, prefix)
        assert h.is_cuda and h.shape == ((K if r else 1), P, 256)
        assert np.array_equal(h.cpu().numpy(), R.hist(x, r, prefix)), r
        seen.append(r)
        return [h]
    comp = _capi.quant_select(hist, PROBS, P)
    assert seen == list(range(8))
    one = ctx.quantiles(t, PROBS)
    again = ctx.quantiles(t, PROBS)
    for k in ("quantiles", "draws_used"):
        assert R.same_bits(one[k], comp[k]) and R.same_bits(one[k], again[k]), k
    assert R.same_bits(one["quantiles"], quant)


def test_one_target_and_sixteen(ctx):
    """K = 1 and K = 16 (eight probabilities), rounds 0 .. 7 with the prefixes the restatement steps to; nine probabilities: two groups"""
    x, _ = inputs("tile_minus_1")
    t = torch.from_numpy(x).to(DEV)
    probs8 = (0.0, 0.01, 0.3, 0.5, 0.5, 0.77, 0.99, 1.0)
    m = np.isfinite(x.reshape(-1, x.shape[2])).sum(0)
    rank, _ = R.plan(m, probs8)
    prefix = np.zeros(rank.shape, dtype=np.uint64)
    R.step([R.hist(x, 0)], 0, prefix, rank)
    for r in range(1, 8):
        want = R.hist(x, r, prefix)
        assert want.shape[0] == 16
        assert np.array_equal(ctx.quant_hist(t, r, prefix).cpu().numpy(), want), r
        assert np.array_equal(ctx.quant_hist(t, r, prefix[5:6]).cpu().numpy(), want[5:6]), r
        R.step([want], r, prefix, rank)
    assert R.same_bits(ctx.quantiles(t, probs8)["quantiles"], R.sorted_stats(x, probs8)[1])
    probs9 = np.linspace(0.0, 1.0, 9)
    assert R.same_bits(ctx.quantiles(t, probs9)["quantiles"], R.sorted_stats(x, probs9)[1])


def test_chain_splits_give_the_same_bits(ctx):
    x, (order, quant, m) = inputs("ar1")
    t = torch.from_numpy(x).to(DEV)
    for splits in ([(0, 40)], [(0, 1), (1, 17), (17, 40)], [(0, 7), (7, 7), (7, 8), (8, 29), (29, 40)]):
        def hist(r, prefix, K):
            return [ctx.quant_hist(t[a:b], r, prefix) if b > a else _capi.quant_identity(K, x.shape[2]) for a, b in splits]
        got = _capi.quant_select(hist, PROBS, x.shape[2])
        assert np.array_equal(got["draws_used"], m) and R.same_bits(got["quantiles"], quant)


def test_refusals_leave_the_context_usable(ctx):
    x, (order, quant, m) = inputs("narrow_tile")
    t = torch.from_numpy(x).to(DEV)
    n, S, P = x.shape
    hist = torch.full((16, P, 256), -3.0, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    pre = np.zeros((16, P), dtype=np.uint64)
    pp = _capi._ptr(pre, _capi._up)
    f = ctx.lib.rmhmc_quant_hist_dev
    for args in ((None, n, S, P, 0, None, 1), (t.data_ptr(), 0, S, P, 0, None, 1), (t.data_ptr(), n, 0, P, 0, None, 1),
                 (t.data_ptr(), n, S, 0, 0, None, 1), (t.data_ptr(), n, S, P, -1, pp, 1), (t.data_ptr(), n, S, P, 8, pp, 1),
                 (t.data_ptr(), n, S, P, 1, pp, 0), (t.data_ptr(), n, S, P, 1, pp, 17), (t.data_ptr(), n, S, P, 0, None, 0),
                 (t.data_ptr(), n, S, P, 1, None, 2)):
        t0 = time.perf_counter()
        assert f(ctx._h, *args, hist.data_ptr()) == -1, args[1:]
        assert time.perf_counter() - t0 < 1.0
    assert "quant_hist_dev" in ctx.lib.rmhmc_last_error(ctx._h).decode()
    assert f(ctx._h, t.data_ptr(), n, S, P, 0, None, 1, None) == -1
    assert (hist == -3.0).all()                                      # nothing was written
    out = np.full((1, P), -3.0)
    g = ctx.lib.rmhmc_quant_dev
    for probs, Q in (([1.5], 1), ([np.nan], 1), ([0.5] * 9, 9), ([0.5], 0)):
        assert g(ctx._h, t.data_ptr(), n, S, P, _capi._ptr(np.array(probs)), Q, _capi._ptr(out), None) == -1
    assert g(ctx._h, t.data_ptr(), n, S, P, None, 1, _capi._ptr(out), None) == -1 and (out == -3.0).all()
    with pytest.raises(ValueError, match="GPU"):
        ctx.quantiles(torch.zeros(2, 8, 3, dtype=torch.float64), 0.5)
    with pytest.raises(ValueError, match="float64"):
        ctx.quant_hist(torch.zeros(2, 8, 3, device=DEV), 0)
    with pytest.raises(ValueError, match="prefix"):
        ctx.quant_hist(t, 1, np.zeros((2, P + 1), dtype=np.uint64))
    assert R.same_bits(ctx.quantiles(t, PROBS)["quantiles"], quant)  # ... and the context works as before


# ---- a sampler: sample_to(quantiles=...) at the size of the australian data ---------------------------------------------------------------
def test_sample_to_with_quantiles(hip):
    M, D, n, n_iter, burn = 690, 15, 6, 50, 20
    XX, t = synthetic_logreg(M, D, 3)
    with hip.context(M, D, n) as c, np.errstate(all="ignore"):
        c.set_data(XX, t)
        t0 = time.perf_counter()
        with pytest.raises(ValueError, match="probabilities"):
            c.sample_to("hmc", 10 ** 6, 10, quantiles=(0.5, 1.5))    # refused before any sampling work
        assert time.perf_counter() - t0 < 1.0
        plain = c.sample_to("hmc", n_iter, burn, samples=True, seed=5)
        host = c.sample_to("hmc", n_iter, burn, samples=True, stats=True, seed=5, quantiles=PROBS)
        dev = c.sample_to("hmc", n_iter, burn, where="device", device=DEV, seed=5, quantiles=0.5, diagnostics=True)
    x = plain["samples"]
    assert set(host) == set(plain) | {"mean", "var", "ess"} | set(_capi.QUANT_KEYS_OUT)
    assert set(dev) == (set(plain) - {"samples"}) | {"diag_partial"} | set(_capi.DIAG_KEYS) | set(_capi.QUANT_KEYS_OUT)
    for k in ("samples", "accepted", "leapfrog_steps"):
        assert isinstance(host[k], np.ndarray) and np.array_equal(host[k], plain[k]), k
    assert dev["accepted"].is_cuda and np.array_equal(dev["accepted"].cpu().numpy(), plain["accepted"])
    _, quant, m = R.sorted_stats(x, PROBS)
    assert (m == n * (n_iter - burn)).all() and np.array_equal(host["quantile_draws"], m)
    assert R.same_bits(host["quantiles"], quant)
    assert dev["quantiles"].shape == (1, D) and R.same_bits(dev["quantiles"][0], quant[2])


# ---- sharded: three gloo ranks on the one GPU ---------------------------------------------------------------------------------------------
def test_sharded_quantiles_under_gloo(hip, tmp_path):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    out = str(tmp_path / "r0.npz")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="3", LOCAL_RANK="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "helpers", "sharded_quant_child.py"), out], cwd=ROOT,
                              env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(3)]
    try:
        logs = [p.communicate(timeout=240)[0] for p in procs]       # every child under a limit of its own
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, p in enumerate(procs):                                    # ... and every exit status checked
        assert p.returncode == 0, (r, logs[r][-3000:])
    g = np.load(out)
    XX, t = synthetic_logreg(child.M, child.D, 3)
    for n_chains, counts in child.CHAINS:
        for name, gather in child.SAMPLERS:
            with hip.context(child.M, child.D, n_chains) as c, np.errstate(all="ignore"):
                c.set_data(XX, t)
                one = c.sample_to(name.lower(), child.N_ITER, child.BURN, samples=True, seed=child.SEED, quantiles=child.PROBS)
            pre = "%s.%d." % (name, n_chains)
            assert np.array_equal(g[pre + "accepted"], one["accepted"])
            if gather == "samples":
                assert np.array_equal(g[pre + "samples"], one["samples"])
            assert np.array_equal(g[pre + "quantile_draws"], one["quantile_draws"])
            assert (one["quantile_draws"] == n_chains * (child.N_ITER - child.BURN)).all()
            assert R.same_bits(g[pre + "quantiles"], one["quantiles"])                 # bit-equal to the one-rank result
            assert R.same_bits(one["quantiles"], R.sorted_stats(one["samples"], child.PROBS)[1])      # ... which is np.sort's
