"""GPU tests of the ESS / mean / variance kernel k_ess (csrc/kernels.hip.h) and the run-mean kernel k_run_mean (csrc/output.hip.h) at
their edges, against ess_ld, the long-double lag-by-lag estimator of tests/helpers/ess_edges.py.  The case table, the references and
the bounds are that helper's; tests/test_ess_edges_cpu.py holds them to their own conditions and shows, on a float64 restatement of the
kernel, that the table tells every named error of a kernel from a right one (a wrap that is ignored or off by one lag, a dropped last
row or lane, the clamp, the stopping rule, the non-finite contract).

Tolerances are the project's (tests/test_gpu_out.py): ESS rtol 1e-9, mean and variance rtol 1e-12 / atol 1e-14; the one exception is
the series about a mean of 1e8 standard deviations (test_offsets).  Everything that can be exact is asserted exact: the entry points
among each other, both modes where no wrapped lag is reached, the ESS of an alternating series (S), powers of two, the place of a
series in its block, the neighbours of a non-finite series, the run mean.

Why an alternating series must return S in linear mode: for a centred series the autocorrelations of all lags l >= 1 sum to -1/2, so
the sum over every pair is 1 - 1/2 = 1/2 for even S and 1/2 - rho_(S-1) <= 1 for odd S; every Gamma_j is about 1 / S > 0, so the sum
runs through every pair, tau = -1 + 2 sum <= 1 is raised to 1 and ESS = S / 1.

Needs an MI355X: run with  pytest -m gpu."""
import os
import sys
import time

import numpy as np
import pytest
import torch

from conftest import GOLDEN, synthetic_logreg
from riemannhamiltonianmontecarlo_amd import _capi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ess_edges as E  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ("linear", "wrap")
OFFSET_IDS = ["offset-%g" % o for o in E.OFFSETS]
TABLE = [c for c in E.CASES if c.id not in OFFSET_IDS]
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ctxs(hip):
    """one context per mode for the whole module (the ESS entry points need no data)"""
    made = {"linear": hip.context(10, 2, 1, flags=0), "wrap": hip.context(10, 2, 1, flags=_capi.FLAG_ESS_WRAP)}
    yield made
    for c in made.values():
        c.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def run_dev(ctx, x):
    """rmhmc_ess_dev on a device copy of x: dict(ess, mean, var) of host arrays"""
    with np.errstate(all="ignore"):
        out = ctx.ess_dev(torch.tensor(np.asarray(x), dtype=torch.float64, device=DEV))
    return {k: t.cpu().numpy() for k, t in zip(("ess", "mean", "var"), out)}


def run_case(ctxs, case):
    """the case through rmhmc_ess (host buffer) and rmhmc_ess_dev (device tensor) of its mode's context, which must agree bit for bit;
    where ess_ld says that no wrapped lag is reached before the sums stop, the other mode's context must agree bit for bit as well"""
    x = E.case_block(case)
    got = run_dev(ctxs[case.mode], x)
    assert same_bits(ctxs[case.mode].ess(x), got["ess"]), case.id
    w = E.case_ref(case, "wrap")
    if (2 * w["pairs"] + 1 < E.nfft_of(case.S, "wrap") - case.S + 1).all():
        other = run_dev(ctxs["wrap" if case.mode == "linear" else "linear"], x)
        for k in got:
            assert same_bits(other[k], got[k]), (case.id, k, "modes")
    return got


def check_case(got, case):
    ref, b = E.case_ref(case), E.case_bounds(case)
    e = E.errors(got, ref)
    print("%s [%s]: ess %.2e (bound %.1e), mean %.2e, var %.2e (units of the tolerance; bounds %.3g, %.3g) | %s"
          % (case.id, case.mode, e["ess"], b["ess"], e["mean"], e["var"], b["mean"], b["var"], case.why))
    assert e["nan"], (case.id, "NaN pattern")
    for k in ("ess", "mean", "var"):
        assert e[k] <= b[k], (case.id, k, e[k], b[k])
    return e


# ---- 1. every case of the table, every entry point -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", TABLE, ids=[c.id for c in TABLE])
def test_table(ctxs, case):
    got = run_case(ctxs, case)
    check_case(got, case)
    if case.gen[0] == "alt" and case.mode == "linear":
        assert (got["ess"] == case.S).all(), got["ess"]
    if case.id.startswith("size-wrap-s") and case.S in E.WRAP_REACHED:
        lin = E.case_ref(case, "linear")["ess"]                    # the wrap is in the numbers: not the linear estimator's
        assert (np.abs(got["ess"] / lin - 1) > 1e-3).mean() >= 0.5


# ---- 2. series about a large mean --------------------------------------------------------------------------------------------------------------
def test_offsets(ctxs):
    """AR(0.7), S = 1000, 20 series about means of 0, 1e4 and 1e8 standard deviations.  The first two: the project's tolerances.  At 1e8
    float64 is itself off - the mean is rounded to 1e8 x 2^-53 = 1.1e-8 sd, and every centred value with it - so the bound is ten times
    the error of the float64 host restatement (tools.CalculateESS, two-pass NumPy mean and variance) against ess_ld on the same inputs.

    Measured, errors against ess_ld at 1e8 sd (ESS relative; mean and variance in units of rtol 1e-12 / atol 1e-14):
      host restatement   ESS 1.45e-09   mean 1.8e-03   var 3.1e-02
      CPU oracle         ESS 8.60e-09   (sequential mean)
      k_ess, MI355X      ESS 1.45e-09   mean 2.1e-04   var 5.7e-04
    so the bound is 1.45e-08 for the ESS and the project's tolerance for mean and variance."""
    for cid in OFFSET_IDS:
        case = E.CASE[cid]
        got = run_case(ctxs, case)
        b = E.case_bounds(case)
        if "host" in b:
            h = b["host"]
            print("%s: host restatement against ess_ld: ess %.2e, mean %.2e, var %.2e" % (cid, h["ess"], h["mean"], h["var"]))
        e = check_case(got, case)
        print("%s: kernel against ess_ld: ess %.2e, mean %.2e, var %.2e" % (cid, e["ess"], e["mean"], e["var"]))


# ---- 3. powers of two ----------------------------------------------------------------------------------------------------------------------------
def test_power_of_two_scaling(ctxs):
    """x 2^k is exact in every product, sum and quotient of the kernel while nothing overflows or goes subnormal.  c0 is about
    2^(2k + 10): normal for every k of the table (2^-590 ... 2^610; tests/test_ess_edges_cpu.py asserts it of ess_ld on the float64
    inputs), so the ESS is bit-identical across all five scales, the mean scales by 2^k and the variance by 4^k, exactly."""
    base = run_case(ctxs, E.CASE[E.SCALE_BASE])
    assert np.isfinite(base["ess"]).all()
    for k in E.SCALES:
        if k == 0:
            continue
        got = run_case(ctxs, E.CASE["scale-2^%d" % k])
        assert all(np.isfinite(got[q]).all() for q in got), k
        assert same_bits(got["ess"], base["ess"]), k
        assert same_bits(got["mean"], base["mean"] * 2.0 ** k), k
        assert same_bits(got["var"], base["var"] * 4.0 ** k) and (got["var"] > 0).all(), k


# ---- 4. the place of a series in its block ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,P", E.PLACE_BLOCKS)
def test_placement_independence(ctxs, n, P):
    """one S = 129 series as column d of chain c among other series: idx / P, idx % P and the stride-P loads"""
    x1 = E.place_series()[None, :, None]
    for mode in MODES:
        alone = run_dev(ctxs[mode], x1)
        ref = E.ess_ld(x1[0], E.nfft_of(E.PLACE_S, mode))
        assert ref["margin"][0] > E.MARGIN and abs(alone["ess"][0, 0] / ref["ess"][0] - 1) <= E.ESS_RTOL
        for c, d in E.placements(n, P):
            got = run_dev(ctxs[mode], E.place_block(n, P, c, d))
            for k in alone:
                assert got[k][c, d].tobytes() == alone[k][0, 0].tobytes(), (mode, n, P, c, d, k, got[k][c, d], alone[k][0, 0])


# ---- 5. non-finite series ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", E.NONFINITE)
@pytest.mark.parametrize("mode", MODES)
def test_non_finite_series(ctxs, kind, mode):
    """a series with a NaN or an inf: ESS, mean and variance NaN, for that series only; a constant one: no ESS, its mean exactly, variance
    0.  Every other series of the block is bit-identical to what it is beside a finite series in that place."""
    case = E.CASE["nonfinite-%s%s" % (kind, "-wrap" if mode == "wrap" else "")]
    assert case.mode == mode
    x, twin = E.case_block(case), E.base_block(case)
    got, clean = run_dev(ctxs[mode], x), run_dev(ctxs[mode], twin)
    assert same_bits(ctxs[mode].ess(x), got["ess"])
    planted = np.zeros((case.n, case.P), dtype=bool)
    c, d = E.PLANT_AT
    if kind == "nan_tail":
        planted[c, :] = True
    else:
        planted[c, d] = True
    assert all(np.isfinite(clean[k]).all() for k in clean)
    for k in got:
        assert same_bits(got[k][~planted], clean[k][~planted]), (kind, mode, k)
    assert np.isnan(got["ess"][planted]).all()
    if kind == "const":
        assert got["mean"][c, d] == E.CONST_VALUE and got["var"][c, d] == 0.0
    else:
        assert np.isnan(got["mean"][planted]).all() and np.isnan(got["var"][planted]).all()


# ---- 6. the reference's own wrap, on the GPU ---------------------------------------------------------------------------------------------------------
def test_s4096_golden_in_wrap_mode(ctxs):
    """S = 4096, the recorded output of the reference's Python (FFT length 4097): where the wrap matters, until now run in wrap mode
    only by the CPU oracle"""
    g = np.load(os.path.join(GOLDEN, "ess_s4096.npz"))
    x = g["samples"]
    got = ctxs["wrap"].ess(x)[0]
    print("ess_s4096, wrap mode: rel err %.2e" % np.abs(got / g["ess"] - 1).max())
    assert np.allclose(got, g["ess"], rtol=1e-9, atol=0)
    assert (np.abs(ctxs["linear"].ess(x)[0] / g["ess"] - 1) > 1e-3).any()


# ---- 7. k_run_mean ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,S,D", E.RUN_MEAN_SHAPES)
def test_run_mean_edges(hip, ctxs, n, S, D):
    """AMH runs whose S D = 255 ... 259 lie on both sides of the 256-thread block and whose chain counts lie on both sides of the chain
    loop's unroll of 8: the run mean is the chains added in order and one division, bit for bit; its ESS is the ESS kernel's on that
    block, bit for bit, and ess_ld's to 1e-9; device and host write-outs are equal."""
    burn = 13
    XX, t = synthetic_logreg(E.RUN_MEAN_M, D, 3)
    with hip.context(E.RUN_MEAN_M, D, n, flags=0) as ctx:
        ctx.set_data(XX, t)
        h = ctx.sample_to("amh", S + burn, burn, samples=True, run_mean=True, seed=17)
        d = ctx.sample_to("amh", S + burn, burn, where="device", device=torch.device(DEV), samples=True, run_mean=True, seed=17)
    x = h["samples"]
    assert x.shape == (n, S, D) and np.isfinite(x).all() and h["run_mean"].shape == (S, D) and h["run_ess"].shape == (D,)
    for k in ("samples", "run_mean", "run_ess"):
        assert same_bits(d[k].cpu().numpy(), h[k]), k
    assert same_bits(h["run_mean"], E.run_mean_def(x))
    assert same_bits(h["run_ess"], ctxs["linear"].ess(h["run_mean"])[0])
    ref = E.ess_ld(h["run_mean"], 0)
    assert (ref["margin"] > E.MARGIN).all(), ref["margin"]
    err = np.abs(h["run_ess"] / ref["ess"] - 1).max()
    print("n %d, S %d, D %d (S D = %d): run_ess against ess_ld %.2e, Geyer margin %.1e" % (n, S, D, S * D, err, ref["margin"].min()))
    assert err <= E.ESS_RTOL


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S_bad", [-1, 0, 1, 20001])
def test_series_length_is_refused_before_anything_is_sized_by_it(hip, ctxs, S_bad):
    """rmhmc_ess and rmhmc_ess_dev: RMHMC_ERR_UNSUPPORTED at once, nothing allocated by S (a non-positive S would wrap the size),
    nothing read or written, and the context works afterwards"""
    ctx = ctxs["linear"]
    n, P = 1, 2
    x = np.zeros((n, 20001, P))                                         # (large enough for every S here: never read)
    out = np.full((n, P), -3.0)
    t0 = time.perf_counter()
    rc = hip.lib.rmhmc_ess(ctx._h, _capi._ptr(x), n, S_bad, P, _capi._ptr(out))
    assert rc == -4 and time.perf_counter() - t0 < 1.0
    assert hip.lib.rmhmc_last_error(ctx._h).decode().startswith("ess: 2 <= S <= 20000")
    assert (out == -3.0).all()
    xd = torch.zeros((n, 20001, P), dtype=torch.float64, device=DEV)
    outs = [torch.full((n, P), -3.0, dtype=torch.float64, device=DEV) for _ in range(3)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = hip.lib.rmhmc_ess_dev(ctx._h, xd.data_ptr(), n, S_bad, P, *[o.data_ptr() for o in outs])
    assert rc == -4 and time.perf_counter() - t0 < 1.0
    assert all((o.cpu().numpy() == -3.0).all() for o in outs)
    case = E.CASE["size-lin-s5"]
    check_case(run_case(ctxs, case), case)


def test_too_many_series_is_refused(hip, ctxs):
    """n P = 2^31 series: RMHMC_ERR_INVALID from both entry points before a pointer is used (the buffers here hold two numbers)"""
    ctx = ctxs["linear"]
    x = np.zeros(2); out = np.full(2, -3.0)
    assert hip.lib.rmhmc_ess(ctx._h, _capi._ptr(x), 2 ** 16, 2, 2 ** 15, _capi._ptr(out)) == -1
    xd = torch.zeros(2, dtype=torch.float64, device=DEV); od = torch.full((2,), -3.0, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    assert hip.lib.rmhmc_ess_dev(ctx._h, xd.data_ptr(), 2 ** 16, 2, 2 ** 15, od.data_ptr(), None, None) == -1
    assert (out == -3.0).all() and (od.cpu().numpy() == -3.0).all()
    case = E.CASE["size-lin-s5"]
    check_case(run_case(ctxs, case), case)
